/* cclip_hip.h - C ABI of libcclip_hip.so: the MI355X (gfx950) kernels behind the CLIP hot path.
 *
 * The reference has no FFI/plugin boundary for this path: its scripts `import clip` and call
 * Python (`model(image, text)`, /root/reference/CLIP/train.py:161; `model.encode_image`,
 * /root/reference/CLIP_prefix_caption/parse_coco.py:43; `model.clip_project` + `model.gpt(...)`,
 * /root/reference/CLIP_prefix_caption/train.py:262,268).  The arithmetic behind those calls is
 * torch ATen kernels reached through the third-party `clip` / `transformers` packages
 * (SURVEY.md 2b).  Each entry point below replaces one group of those ATen launches; the
 * Python `clip` drop-in in construction-clip_amd/ binds them with ctypes.
 *
 * Conventions: every pointer is a DEVICE pointer unless stated; `stream` is a hipStream_t
 * (torch.cuda.current_stream().cuda_stream on ROCm); all launches are asynchronous and
 * graph-capturable (no allocation, no synchronisation inside); workspaces come from the caller.
 * Return value: 0 = CCLIP_OK, 1 = argument/shape/alignment contract violated (nothing was
 * launched), 2 = HIP launch error.  The Python shim maps non-zero to RuntimeError.
 * bf16 buffers are passed as `void*` (raw 16-bit storage, torch.bfloat16).
 */
#ifndef CCLIP_HIP_H
#define CCLIP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define CCLIP_ABI_VERSION 3
int cclip_abi_version(void);

/* ---- epilogue activations (forward and their backward forms) ---- */
enum {
  CCLIP_ACT_NONE = 0,
  CCLIP_ACT_QUICKGELU = 1, /* x*sigmoid(1.702x): CLIP ResidualAttentionBlock MLP */
  CCLIP_ACT_TANH = 2,      /* prefix mapper, CLIP_prefix_caption/train.py:115-123 */
  CCLIP_ACT_GELU_NEW = 3,  /* GPT-2 MLP */
  CCLIP_ACT_RELU = 4,      /* TransformerMapper MLP, CLIP_prefix_caption/train.py:126-140 */
  /* backward forms: out = acc * act'(aux); aux = saved pre-activation (saved OUTPUT for tanh) */
  CCLIP_ACT_DQUICKGELU = 16,
  CCLIP_ACT_DTANH = 17,
  CCLIP_ACT_DGELU_NEW = 18,
  CCLIP_ACT_DRELU = 19
};

/* ---- bf16 MFMA GEMM:  C[m][n] = epi(alpha * sum_k A(m,k) B(n,k)) --------------------------
 * Replaces nn.Linear / nn.MultiheadAttention projections / Conv1D / lm_head matmuls and their
 * dgrad + wgrad.  a_kcontig: A(m,k) at A[m*lda+k] (1) or A[k*lda+m] (0); b_kcontig: B(n,k) at
 * B[n*ldb+k] (1) or B[k*ldb+n] (0).  Supported (a,b): (1,1) forward, (1,0) dgrad / Conv1D,
 * (0,0) wgrad.  Contract: lda, ldb, ldc (and ldr % 4, ldaux % 8) multiples of 8 elements and every row
 * readable up to the next multiple of 8 columns (pad the leading dimension; e.g. a vocabulary of
 * 50257 uses ld 50264) - M, N and K themselves are arbitrary; when K is not a multiple of 8 the pad
 * columns of a K-contiguous operand up to the next multiple of 8 must hold finite values (the other
 * operand's matching k-rows are zero-filled by the kernel);
 * A and B 16-byte aligned.  Epilogue order: *alpha, +bias[n], (store out_pre_bf16), act,
 * +residual[m][n] (fp32, may alias out_f32), store out_f32 and/or out_bf16.
 * split_k > 1: K is cut into split_k ranges whose fp32 partial tiles go to split_ws
 * (>= split_k*M*N floats) and are summed by a second launch (bias/act/out_pre must be unset). */
typedef struct cclip_gemm_desc {
  const void* A;
  const void* B;
  int32_t a_kcontig, b_kcontig;
  int64_t lda, ldb;
  int32_t M, N, K;
  float alpha;
  const float* bias;
  int32_t act;
  const void* aux;
  int64_t ldaux;
  const float* residual;
  int64_t ldr;
  float* out_f32;
  void* out_bf16;
  void* out_pre_bf16;
  int64_t ldc;
  int32_t split_k;
  float* split_ws;
  int32_t tile_config; /* 0 = auto (128x128; M <= 8 rows against K-strided weights takes the skinny GEMV path);
                        * 1 = 128x128 tile, 2 LDS stages; 2 = 256x128, 3 stages; 3 = 256x256, 2 stages;
                        * 4 = persistent 256x128 with the epilogue streamed under the next tile's K loop - forward layout,
                        *     M % 256 == 0, N % 128 == 0, N <= 4096, K >= 512 (640 with a residual), one of the three
                        *     epilogue forms {16-bit out | pre-activation + activation | fp32 out + residual}; status 1 otherwise.
                        * 5 = 192x256 (configuration 3's K loop with 96x64 per wave; K-contiguous A only): a tile-count
                        *     quantisation option - 9.39 rounds of 0.75-size tiles instead of 7.03 rounds of full ones.
                        * 7 = configuration 3 with the ROTATED K loop (k-step 1 of the previous K-tile is multiplied right after the
                        *     barrier while the new tile's fragments are read) - forward layout only; status 1 otherwise.
                        * 8 = 256x256 run by FOUR waves of 128x128 (one per SIMD, accumulators in AGPRs) with a hand-scheduled inline-asm
                        *     K loop (tools/gen_gemm_a4.py) and an LDS-staged epilogue that stores whole 256-byte row segments;
                        *     forward layout, K % 64 == 0, K >= 128, no split-K; status 1 otherwise.
                        * 10 = configuration 8 as a persistent kernel (one work-group per CU walks tiles, the next tile's first operands
                        *     are staged during the current tile's last iteration); K >= 192.  Not an autotuner candidate: next to a
                        *     second stream's kernels it loses to configuration 8 (it holds every CU for its whole life).
                        * 11 = the WEIGHT-GRADIENT layout (a_kcontig = b_kcontig = 0: both operands strided in K) on four 128x128 waves
                        *     with a hand-scheduled K loop (transposing LDS reads; tools/gen_gemm_a4.py), split-K, fused colsum_out
                        *     (of A; colsum_of_b is refused); M, N multiples of 8, K % 64 == 0 and at least two 64-deep K-tiles per
                        *     split (callers keep activation / gradient slabs on 64-row multiples with zero tails); status 1 otherwise.
                        * Bits 8..15 (configurations 1, 2, 3, 5, 7, 8): TILE ORDER - 0 = row-major over (row tile, column tile);
                        *     G > 0 = the column tiles in groups of G, every row tile of a group before the next group.  Work-items
                        *     that run together on one XCD then share G weight panels instead of all of them: a weight wider than
                        *     an XCD's L2 (N = 3072 at K = 768: 4.7 MB) stays resident (fc projection -8 %, 8192^3 -29 %).
                        *     Same tiles, same arithmetic per tile: bit-identical output.
                        * The host-side autotuner (cclip_hip/ops.py) times the configurations per shape. */
  /* wgrad layout (0,0) only: colsum_out[m] (+)= sum_k A(m,k) - the BIAS gradient of the layer whose weight gradient this
   * call computes (A = dY^T), taken off the operand tiles already in LDS by one extra MFMA per m-tile against an all-ones
   * fragment in the first column block of tiles.  With split_k > 1 split_ws must hold split_k*M*(N+1) floats. */
  float* colsum_out;
  int32_t colsum_accumulate;
  int32_t colsum_of_b;   /* 1: colsum_out[n] (+)= sum_k B(n,k) instead (size N; first ROW block of tiles) - the Conv1D weight layout,
                          * where dY is the B operand of the weight-gradient GEMM; workspace split_k*(M*N + max(M,N)) floats */
  /* ---- LayerNorm FOLDED into the projection that follows it (tile configuration 8; M % 256 == 0, N % 256 == 0) ----
   * LayerNorm(x) W^T + b  =  rstd_m * ( x W'^T - mean_m * c1_n ) + c2_n   with W' = gamma (.) W, c1_n = sum_k W'(n,k),
   * c2_n = b_n + sum_k beta_k W(n,k): A holds the UN-normalised rows as 16-bit values, B holds W', `bias` holds c2,
   * ln_stats = fp32 [M][2] (mean, rstd) of the rows, ln_c1 = fp32 [N].  Epilogue: v = rstd*(alpha*acc - mean*c1) + bias, then act. */
  const float* ln_stats;
  const float* ln_c1;
  /* The residual-stream form (out_f32 = alpha*acc + bias + residual) may emit what the NEXT folded projection needs: out_bf16 (a
   * 16-bit copy of the new rows; allowed next to out_f32 + residual for these configurations) and rowstats_out = fp32
   * [N/64][M][2]: (sum, sum of squares) of every new row over each 64-column block, combined by cclip_rowstats_combine. */
  float* rowstats_out;
} cclip_gemm_desc;
int cclip_gemm_bf16(const cclip_gemm_desc* d, hipStream_t stream);
/* stats[m] = (mean, rstd = rsqrt(var + eps)) of row m from nblk partial (sum, sum of squares) pairs: partials fp32 [nblk][rows][2] */
int cclip_rowstats_combine(const float* partials, int32_t nblk, int32_t rows, int32_t D, float eps, float* stats, hipStream_t stream);

/* ---- LayerNorm (fp32 statistics, eps as given) ---------------------------------------------
 * Replaces nn.LayerNorm (ln_pre / ln_1 / ln_2 / ln_post / ln_final; GPT-2 ln_1 / ln_2 / ln_f).
 * x: fp32 rows of D (row stride ldx); row r of the output normalises input row
 * (row_index ? row_index[r] : r) - the index form is the pooled `ln_post(x[:,0])` /
 * `ln_final(x)[n, argmax]`.  Outputs: bf16 and/or fp32 [rows, D] (row stride ldo), optional
 * mean[rows], rstd[rows] for backward.  D % 4 == 0, D <= 1024. */
int cclip_layernorm_fwd(const float* x, int64_t ldx, const int32_t* row_index, int32_t rows, int32_t D,
                        const float* gamma, const float* beta, float eps, void* out_bf16, float* out_f32,
                        int64_t ldo, float* mean, float* rstd, hipStream_t stream);
/* Backward.  dy: [rows, D] bf16 (dy_is_bf16) or fp32.  dx is written at the *input* row
 * (row_index applied): dx_out[src] = (dx_res ? dx_res[src] : 0) + dLN; optional bf16 copy.
 * dgamma/dbeta (both or neither): column sums over rows, `accumulate` adds to existing values;
 * ws must hold cclip_layernorm_bwd_ws_floats(rows, D) floats. */
int cclip_layernorm_bwd_ws_floats(int32_t rows, int32_t D);
int cclip_layernorm_bwd(const void* dy, int32_t dy_is_bf16, int64_t lddy, const float* x, int64_t ldx,
                        const int32_t* row_index, int32_t rows, int32_t D, const float* gamma,
                        const float* mean, const float* rstd, const float* dx_res, float* dx_out,
                        void* dx_out_bf16, int64_t lddx, float* dgamma, float* dbeta, int32_t accumulate,
                        float* ws, hipStream_t stream);

/* ---- fused multi-head attention, head_dim 64, T <= 8192, forward and backward ------------------
 * (T > 128 - ViT-B/16 197, ViT-L/14 257, ViT-L/14@336px 577 tokens - runs the key-block-tiled
 * online-softmax forward and a two-launch backward: dK/dV per key block, dQ per query block.)  Replaces softmax(q k^T * scale + mask) v of nn.MultiheadAttention (CLIP towers; causal for the
 * text tower) and of GPT-2 (causal + key padding).  q/k/v/o/d*: bf16, row (b*T + t), head h at
 * column h*64 of the given base pointer (so a packed [B*T, 3D] qkv buffer is passed as three
 * offset pointers with the same row stride).  lse: fp32 [B,H,T] written by fwd, read by bwd.
 * key_keep: optional fp32 [B,T], 0 masks a key.  Backward needs o (for rowsum(dO*O)). */
typedef struct cclip_attn_desc {
  const void* q; const void* k; const void* v;
  int64_t ldq, ldk, ldv;
  void* o; int64_t ldo;
  float* lse;
  const float* key_keep;
  int32_t B, T, H, head_dim, causal;
  float scale;
  const void* dout; int64_t lddo;
  void* dq; void* dk; void* dv;
  int64_t lddq, lddk, lddv;
  /* cclip_attention_fwd only (round 2, fp8 inference path): o_fp8 != NULL -> the output rows are written as e4m3 [B*T, H*64]
   * (row stride ldo_fp8) + E8M0 block scales in cclip_quantize_mx_fp8's layout (plane stride ld_o_block_scale >= 4*B*T) - the
   * block-scaled A operand of the out-proj GEMM (cclip_gemm_fp8_ex), with no 16-bit round trip; o is then not written. */
  void* o_fp8; int64_t ldo_fp8; void* o_block_scale; int64_t ld_o_block_scale;
  /* packed (variable-length) batches (round 2; cclip_attention_fwd / _bwd, T <= 128): cu_seqlens != NULL (int32 [B+1], device) ->
   * sequence b occupies rows [cu[b], cu[b+1]) of q/k/v/o/d* and of key_keep, T = the longest length (lse keeps row stride T).
   * The text tower's captions end at their EOT token: rows after it never influence the pooled feature (causal attention), so
   * the tower runs on sum(len) rows instead of B*77. */
  const int32_t* cu_seqlens;
} cclip_attn_desc;
int cclip_attention_fwd(const cclip_attn_desc* d, hipStream_t stream);
int cclip_attention_bwd(const cclip_attn_desc* d, hipStream_t stream);
/* Attention relevance of one layer (Chefer et al.; the step of the reference's interpret(), attention.py:14-69), T <= 128:
 * C = 1 / (H grad_scale) sum_h max(P_h (.) dP_h, 0) with P_h = exp(scale Q_h K_h^T - lse_h) (causal / lengths as in
 * cclip_attention_bwd) and dP_h = dA_h V_h^T, then R[:T_b, :T_b] += R[:T_b, :T_b] C per sequence; the rest of R is not touched.
 * Reads q, k, v, lse, B, T, H, causal, scale, cu_seqlens of d; dA is d->dout / d->lddo (the gradient at the attention output,
 * as for the backward).  R: fp32 [B, T, T], updated in place.  grad_scale > 0: the loss scale the dgrad chain runs under.
 * Neither P nor dP is written anywhere. */
int cclip_attention_relevance(const cclip_attn_desc* d, float grad_scale, float* R, hipStream_t stream);
/* One row of the same step, 1 <= T <= 8192 (the long towers: ViT-B/16 197, ViT-L/14 257, ViT-L/14@336px 577 tokens): the row
 * vector r of R obeys r <- r + r C, so per sequence b of length T_b (T, or cu[b+1] - cu[b] clamped to T; lse keeps row stride T)
 *   r_out[b, j] = r_in[b, j] + 1 / (H grad_scale) sum_{i < T_b} r_in[b, i] sum_h max(P_h[i, j] dP_h[i, j], 0)     (j < T_b)
 *   r_out[b, j] = r_in[b, j]                                                                                      (T_b <= j < T)
 * with P_h, dP_h and the fields read from d as for cclip_attention_relevance.  r_in, r_out: fp32 [B, T] contiguous and DIFFERENT
 * buffers (a workgroup reads all of r_in[b] while others write r_out[b]).  Neither P, dP nor C is written to memory; no atomics:
 * two launches agree bit for bit.  CCLIP_ERR_ARG, with no launch, for null pointers, r_in == r_out, head_dim != 64,
 * grad_scale <= 0, a leading dimension that is no multiple of 8, or q / k / v / dout not 16-byte aligned. */
int cclip_attention_relevance_row(const cclip_attn_desc* d, float grad_scale, const float* r_in, float* r_out, hipStream_t stream);
/* Attention probabilities of one layer, T <= 256 (what HF's `output_attentions=True` returns; the reference's generate_beam
 * logs them, CLIP_prefix_caption/test.py:381-390): P[b, h, i, 0:T] = softmax_j(scale q_t k_j + mask) in fp32 for the query
 * position t = q_rows[i] (q_rows: optional int32 DEVICE array of n_q positions shared by all sequences, values clamped to
 * 0 .. T-1; NULL = all T positions, n_q is then ignored).  Element (b, h, i, j) is at P[b*ld_p_b + h*ld_p_h + i*ld_p_q + j],
 * ld_p_q >= T.  Reads q, k, ldq, ldk, B, T, H, head_dim (64), causal, scale, key_keep of d (cu_seqlens must be NULL); lse is
 * NOT read - the row maximum and sum are formed in registers from the scores themselves.  Entries above the causal diagonal
 * and entries of keys with key_keep == 0 are exactly 0 (a row that sees no key is all zeros); every element 0 .. T-1 of a
 * produced row is written, nothing else is.  T > 256 returns CCLIP_ERR_ARG. */
int cclip_attention_probs(const cclip_attn_desc* d, const int32_t* q_rows, int32_t n_q, float* P, int64_t ld_p_b,
                          int64_t ld_p_h, int64_t ld_p_q, hipStream_t stream);
/* Generic small attention for the reference's TransformerMapper (CLIP_prefix_caption/train.py:141-171: 8 heads of
 * 96 over 40 tokens): any head_dim <= 128 (multiple of 8), T <= 64, no mask; same descriptor; LDS must hold one
 * (batch, head): 4*T*(head_dim+2) + 2*T*(T+1) + T floats <= 160 KiB in backward. */
int cclip_attention_small_fwd(const cclip_attn_desc* d, hipStream_t stream);
int cclip_attention_small_bwd(const cclip_attn_desc* d, hipStream_t stream);

/* Decode-shaped attention (head_dim 64): one new query per sequence against its KV cache - the step of the
 * KV-cached replacement for the reference's generate_beam / generate2 loops, which re-run GPT-2 on the whole
 * growing sequence every step (CLIP_prefix_caption/test.py:381,468; application.py:180).  q/out: [B, >= H*64]
 * 16-bit; kcache/vcache: position s of sequence b at element offset b*ld_seq + s*ld_pos, head h at +h*64;
 * S = number of cached positions INCLUDING the new token's own (<= 2048).  No mask (the newest token sees all).
 * ld_pos, ld_seq, ldo multiples of 8 elements; kcache, vcache, out 16-byte aligned (CCLIP_ERR_ARG otherwise). */
int cclip_attention_decode(const void* q, int64_t ldq, const void* kcache, const void* vcache, int64_t ld_pos,
                           int64_t ld_seq, void* out, int64_t ldo, int32_t B, int32_t H, int32_t S, float scale,
                           hipStream_t stream);

/* ---- exact fp32 GEMM (f32-input MFMA), generic strides ---------------------------------------
 * C[m*ldc+n] = alpha' * sum_k A[m*sam + k*sak] * B[n*sbn + k*sbk] + beta * C[m*ldc+n], with
 * alpha' = alpha * (alpha_log_dev ? exp(*alpha_log_dev) : 1)  (logit_scale.exp() without a host sync).
 * Replaces `x @ visual.proj`, `x @ text_projection`, `logit_scale.exp() * I @ T.t()` of
 * CLIP.forward/encode_* and their backward products (tiny, accuracy critical).
 * beta == 0: C is an output only - it is not read, so NaN or uninitialised memory in it does not reach the result.
 * alpha' == 0 does not skip the product: a NaN or inf in A or B still reaches C. */
int cclip_gemm_f32(const float* A, int64_t sam, int64_t sak, const float* B, int64_t sbn, int64_t sbk,
                   int32_t M, int32_t N, int32_t K, float alpha, const float* alpha_log_dev, float beta,
                   float* C, int64_t ldc, hipStream_t stream);

/* ---- embeddings ------------------------------------------------------------------------------
 * cclip_patchify: image fp32 [B,3,R,R] -> bf16 im2col [B*T, 3*P*P], T = (R/P)^2 + 1, class slot
 *   row (t = 0) zero; column order (c, ky, kx) = conv1.weight.view(W,-1).  When 3*P*P is not a
 *   multiple of 8 (P = 14: 588) rows are zero-padded to round_up(3*P*P, 8) elements (592) so they stay
 *   16-byte aligned for the GEMM; pad the weight rows the same way.
 *   Replaces the input side of VisionTransformer.conv1 (k = s = P, no bias).
 * cclip_vit_embed_ln: x0 = patch_out + positional_embedding[t] (+ class_embedding at t = 0),
 *   x = ln_pre(x0); optional saves x0, mean, rstd.  All fp32 [rows = B*T, D].
 * cclip_text_embed: x[r] = token_embedding[text[r]] + positional_embedding[r % L] (pos may be NULL).
 *   Token ids outside [0, V) are clamped to the nearest end of the table by the kernels of cclip_text_embed, cclip_caption_embed
 *   and cclip_embed_scatter_add (never an out-of-bounds access; tests/test_kernels_f32_gpu.py pins it).  The deterministic
 *   gradient does NOT clamp at this level: cclip_embed_tables / cclip_embed_segsum take tok_sorted as given and require ids in
 *   [0, V] (V itself = a dropped row; a negative id would index demb out of bounds) - the host wrapper
 *   (cclip_hip/ops.py embed_scatter_tables) clamps to [0, V - 1] before it sorts.
 * cclip_embed_scatter_add: ids are [n, L]; demb[text[r]] += dx[(r/L)*seq_stride + seq_off + r%L]  (fp32 atomics - hardware
 *   order, kept as the one-launch alternative; the default host path uses cclip_embed_segsum below;
 *   text tower: L = seq_stride = 77, seq_off = 0; caption model: the token part of a longer sequence).
 * cclip_caption_embed: x[b,s] = (s < P ? prefix_proj[b,s] : wte[ids[b,s-P]]) + wpe[s] - the
 *   `cat(clip_project(prefix), wte(cat(attribute,tokens)))` + GPT-2 position add of
 *   CLIP_prefix_caption/train.py:258-263,268.  cclip_add_positional: x = inputs_embeds + wpe[s].
 * cclip_colsum: out[c] (+)= sum_r in[r*ld + c]; in bf16 (ld % 8 == 0) or fp32 (ld % 4 == 0), 16-byte
 *   aligned; C % 4 == 0; deterministic;
 *   ws >= cclip_colsum_ws_floats(R, C) floats. */
int cclip_patchify(const float* image, void* out_bf16, int32_t B, int32_t R, int32_t P, hipStream_t stream);
int cclip_vit_embed_ln(const float* patch_out, const float* cls, const float* pos, int32_t rows, int32_t T,
                       int32_t D, const float* gamma, const float* beta, float eps, float* x0, float* x,
                       float* mean, float* rstd, hipStream_t stream);
int cclip_text_embed(const int32_t* text, const float* emb, const float* pos, int32_t rows, int32_t L,
                     int32_t D, int32_t V, float* x, hipStream_t stream);
int cclip_embed_scatter_add(const int32_t* text, const float* dx, int64_t lddx, int32_t rows, int32_t D,
                            int32_t V, float* demb, int32_t L, int32_t seq_stride, int32_t seq_off,
                            hipStream_t stream);
/* Deterministic form of the same sum (no atomics).  `order` lists the n rows sorted by token id (stable), tok_sorted their ids;
 * per list position p: cend[p] > 0 marks the start of a CHUNK (at most 64 rows of one id) ending at cend[p], cidx[p] is the
 * chunk's slot in `partial`, rlen[p] > 0 marks the start of a run of equal ids made of rlen[p] chunks.
 * One-chunk runs are added into demb[id] by the wave that owns them, longer runs through ordered partials (two launches).
 * All tables are fixed-size index vectors: the caller needs no host synchronisation.  Bit-identical from run to run.
 * cclip_embed_tables builds cend / cidx / rlen from tok_sorted alone (ids >= V = rows dropped up front, sorted to the end):
 * chunk slots are id + (chunk start >> 6), so `partial` holds (V + n/64 + 1) * D floats. */
int cclip_embed_tables(const int32_t* tok_sorted, int32_t n, int32_t V, int32_t* cend, int32_t* cidx, int32_t* rlen,
                       hipStream_t stream);
int cclip_embed_segsum(const int32_t* order, const int32_t* tok_sorted, const int32_t* cend, const int32_t* cidx,
                       const int32_t* rlen, int32_t n, const float* dx, int64_t lddx, int32_t D, float* demb, int32_t L,
                       int32_t seq_stride, int32_t seq_off, float* partial, hipStream_t stream);
int cclip_caption_embed(const float* prefix_proj, const int32_t* ids, const float* wte, const float* wpe,
                        int32_t B, int32_t P, int32_t Lt, int32_t D, int32_t V, float* x, hipStream_t stream);
int cclip_add_positional(const float* emb, const float* wpe, int32_t rows, int32_t S, int32_t D, float* x,
                         hipStream_t stream);
int cclip_colsum_ws_floats(int32_t R, int32_t C);
int cclip_colsum(const void* in, int32_t in_is_bf16, int64_t ld, int32_t R, int32_t C, float* out,
                 int32_t accumulate, float* ws, hipStream_t stream);

/* ---- image features -> zero-shot heads -> attribute ids (CLIP_prefix_caption/test.py:521-542) -----------------
 * One launch for N feature rows feat [N, E] fp32 (row stride ldf, as encode_image returns them: not normalised) against
 * the text features prompts [K, E] fp32 of G heads laid one after another (as encode_text returns them; the kernel
 * normalises them).  head_start is a HOST array of G + 1 ints read during the call: head g owns prompt rows
 * [head_start[g], head_start[g+1]), head_start[0] = 0, head_start[G] = K.  With K_g the size of head g:
 *   logit[n,k] = exp(*logit_scale_dev) * <feat_n, prompt_k> / (|feat_n| |prompt_k|)
 *   probs[n,k] = exp(logit[n,k]) / sum_{j in head(k)} exp(logit[n,j])                                   fp32 [N, K]
 *   index[n,g] = arg-max of logit[n, head g], counted from the head's first row, the LOWEST on a tie   int32 [N, G]
 *   ids[n,:]   = table[((index[n,0] * K_1) + index[n,1]) * K_2 + ...]                                   int32 [N, A]
 * table: int32 [table_rows, A] on the device with table_rows = prod_g K_g (head 0 slowest).  fp32 arithmetic in a fixed
 * order (no atomics): two launches are bitwise equal.  CCLIP_ERR_ARG: a null pointer; N, E, K, G or A <= 0; G > 16; a head
 * with no prompts; table_rows != prod_g K_g; E % 4, E > 1024, ldf < E, ldf % 4, feat or prompts not 16-byte aligned;
 * (K * E + 4 K) floats above 64 KiB (the prompt rows live in LDS).  It touches no 16-bit operand: one form, no _f16 twin. */
int cclip_caption_prompt(const float* feat, int64_t ldf, int32_t N, int32_t E, const float* prompts, int32_t K,
                         const int32_t* head_start, int32_t G, const float* logit_scale_dev, const int32_t* table,
                         int32_t table_rows, int32_t A, float* probs, int32_t* index, int32_t* ids, hipStream_t stream);

/* ---- exact top-k retrieval over stored embeddings (csrc/embed_topk.hip) ---------------------------------------
 * For queries q [Q, D] and a gallery g [N, D], both bf16 (fp16 in the twin) with row strides ldq / ldg in elements, the
 * k largest s[i, n] = sum_d q[i, d] g[n, d] of every query, fp32 accumulation on the MFMA:
 *   scores[i, j]  fp32 [Q, k] contiguous, descending          index[i, j]  int32 [Q, k]: the gallery row of scores[i, j]
 * Exact, not approximate, and the Q x N matrix is never written.  Order: higher score first; equal fp32 scores (-0 == +0)
 * by the LOWER gallery index; a NaN score ranks below every number.  A pair's score does not depend on where the gallery
 * row sits (identical gallery rows give bitwise identical scores), and there are no atomics: the result does not depend
 * on how the launcher splits the gallery, and two launches are bitwise equal.
 * Two launches on `stream`: per-split selection into `workspace`, then the merge.  workspace: at least
 * cclip_similarity_topk_workspace(Q, N, k) bytes (0 for arguments the call would refuse), 8-byte aligned, device memory
 * the caller owns; its contents before and after are meaningless.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): a null pointer; Q <= 0; N <= 0 or N >= 2^31; k < 1, k > 64 or k > N; D <= 0, D % 32
 * or D > 1024; ldq or ldg below D or not a multiple of 8; q or g not 16-byte aligned; workspace too small or misaligned. */
int64_t cclip_similarity_topk_workspace(int32_t Q, int64_t N, int32_t k);
int cclip_similarity_topk(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                          int32_t k, float* scores, int32_t* index, void* workspace, int64_t workspace_bytes,
                          hipStream_t stream);

/* The biased form: the exact top-k of t[i, n] = fmaf(scale, s[i, n], bias[n]) with bias fp32 [N] on the device (4-byte aligned)
 * and s the score above (same bits).  scores holds t.  Same key order on t: higher t first, equal t by the LOWER gallery
 * index, NaN last.  bias[n] = -inf excludes row n: it appears only once the finite rows run out, and then by ascending
 * index (before any NaN).  scale = 1 with bias = 0 returns what cclip_similarity_topk returns, bit for bit.  Same workspace
 * (cclip_similarity_topk_workspace), same two launches (the merge kernel is shared), same refusals, plus a null or
 * misaligned bias. */
int cclip_similarity_topk_biased(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                                 int32_t k, const float* bias, float scale, float* scores, int32_t* index, void* workspace,
                                 int64_t workspace_bytes, hipStream_t stream);

/* ---- how strongly a bank of queries points at every stored row (csrc/embed_hub.hip) -----------------------------
 * For the gallery g [N, D] and the bank [B, D], both bf16 (fp16 in the twin) under the operand contract of
 * cclip_similarity_topk (row strides ldg / ldb in elements), and a float beta:
 *   lse[j] = log sum_{b < B} exp(beta * s[b, j])      fp32 [N],   s[b, j] = sum_d bank[b, d] g[j, d]
 * with s the bits cclip_similarity_topk returns for the pair and beta * s one fp32 multiply.  The B x N matrix is never
 * written.  The sum runs on running (max, sum of exp(t - max)) pairs: nothing above exp(0) is formed, so a large beta stays
 * finite.  B = 1 returns beta * s exactly.  A NaN in gallery row j makes lse[j] NaN and touches no other entry; a non-finite
 * bank row reaches every entry.  No atomics: two launches are bitwise equal.
 * Two launches on `stream`: per-split pairs into `workspace` ([N][splits] pairs of floats, splits =
 * cclip_bank_lse_splits(N, B), at least cclip_bank_lse_workspace(N, B) = 8 N splits bytes, 8-byte aligned, device memory the
 * caller owns), then the merge in ascending split order.  Both queries return 0 for sizes the call would refuse.
 * CCLIP_ERR_ARG (nothing launched): a null pointer; N or B <= 0 or >= 2^31; D <= 0, D % 32 or D > 1024; ldg or ldb below D
 * or not a multiple of 8; g or bank not 16-byte aligned; workspace too small or misaligned; lse not 4-byte aligned. */
int32_t cclip_bank_lse_splits(int64_t N, int64_t B);
int64_t cclip_bank_lse_workspace(int64_t N, int64_t B);
int cclip_bank_lse(const void* g, int64_t ldg, int64_t N, const void* bank, int64_t ldb, int64_t B, int32_t D, float beta,
                   float* lse, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- fixed-radius search over stored embeddings (csrc/embed_range.hip) --------------------------------------
 * For the operands of cclip_similarity_topk (same contract, same score bits per pair): every pair (i, n) with
 * s[i, n] >= threshold, in CSR form.  A NaN score is never a hit, +inf is one; threshold = -inf returns every non-NaN pair.
 *   index[offsets[i] .. offsets[i+1])   int32: the gallery rows of query i, ASCENDING        scores: fp32 alongside
 * self_join = 1 (needs q == g, ldq == ldg, Q == N) keeps only the pairs n > i and skips the tiles that hold none.
 * The Q x N matrix is never written; no atomics: two launches are bitwise equal.  Three steps, the middle one the caller's:
 *   1. cclip_similarity_range_count fills counts, int32 [Q][splits] with splits = cclip_similarity_range_workspace(Q, N) /
 *      (4 Q): the hits of every (query row, gallery split).  counts: that many bytes of device memory, 4-byte aligned.
 *   2. The caller scans: starts[j] = counts[0] + .. + counts[j-1] over the Q * splits counts in memory order, int64 on the
 *      device, and total = their sum, read to the host to size the outputs.  offsets[i] = starts[i * splits],
 *      offsets[Q] = total.
 *   3. cclip_similarity_range_emit (same q, g, threshold, self_join) recomputes the tiles and writes every segment at its
 *      start.  H: the entries index and scores hold; total > H is refused, and no entry at or beyond H is ever written.
 *      total == 0 launches nothing.
 * CCLIP_ERR_ARG (nothing launched): a null pointer; Q <= 0; N <= 0 or N >= 2^31; D <= 0, D % 32 or D > 1024; ldq or ldg
 * below D or not a multiple of 8; q or g not 16-byte aligned; self_join not 0 / 1, or 1 with q != g, ldq != ldg or Q != N;
 * counts too small or misaligned; starts not 8-byte aligned; total < 0, H < 0 or total > H. */
int64_t cclip_similarity_range_workspace(int32_t Q, int64_t N);
int cclip_similarity_range_count(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                                 float threshold, int32_t self_join, int32_t* counts, int64_t workspace_bytes,
                                 hipStream_t stream);
int cclip_similarity_range_emit(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                                float threshold, int32_t self_join, const int64_t* starts, int64_t total, int64_t H,
                                int32_t* index, float* scores, hipStream_t stream);

/* ---- lm_head scoring without the logits (csrc/lm_score.hip) ----------------------------------------------------
 * For hidden rows x [R, D] (the ln_f output) and the vocabulary matrix w [V, D] (the tied wte), both bf16 (fp16 in the twin)
 * with row strides ldx / ldw in elements and inner stride 1, with z[r, j] = sum_d x[r, d] w[j, d] accumulated in fp32 on the MFMA:
 *   lse[r]        = log sum_j exp z[r, j]
 *   logp[r]       = z[r, labels[r]] - lse[r]; exactly 0.0f where labels[r] == ignore_index (checked first); NaN where the
 *                   label lies outside [0, V) (nothing is read out of range)
 *   pred[r]       = argmax_j z[r, j]: equal fp32 logits (-0 == +0) go to the LOWER column, a NaN logit ranks below every number
 *   pred_logit[r] = that maximum
 * all [R] contiguous; lse, pred and pred_logit may be NULL.  The R x V logits are never written.  Every logit is one
 * accumulator chain over d, the vocabulary is split by a rule that depends on V alone and partials are combined in a fixed
 * order without atomics: two launches are bitwise equal, and a row's outputs do not depend on R or on the row's position.
 * Two launches on `stream`: per-split partials into `workspace`, then the merge.  workspace: at least
 * cclip_lm_head_score_workspace(R, V) bytes (0 for arguments the call would refuse; 24 bytes per row and 1024 columns),
 * 8-byte aligned device memory the caller owns; its contents before and after are meaningless.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): null x, w, labels, logp or workspace; R <= 0; V <= 0; D < 32, D % 32 or D > 1024; ldx or
 * ldw below D or not a multiple of 8; x or w not 16-byte aligned; a misaligned output or workspace. */
int64_t cclip_lm_head_score_workspace(int32_t R, int32_t V);
int cclip_lm_head_score(const void* x, int64_t ldx, int32_t R, int32_t D, const void* w, int64_t ldw, int32_t V,
                        const int32_t* labels, int32_t ignore_index, float* logp, float* lse, int32_t* pred,
                        float* pred_logit, void* workspace, hipStream_t stream);

/* ---- class affinities of a few-shot cache model (csrc/embed_cache.hip) -------------------------------------------
 * For queries q [Q, D] and stored rows g [Np, D], both bf16 (fp16 in the twin) with row strides ldq / ldg in elements and
 * inner stride 1, with s[i, n] = sum_d q[i, d] g[n, d] accumulated in fp32 on the MFMA (one chain over d = 0, 32, ..):
 *   out[i, c] = sum over the live rows n of class c with n != exclude[i] of exp(beta * (s[i, n] - 1))     fp32 [Q, C] contiguous
 * The stored rows are grouped by class: class c owns the rows class_off[c] .. class_off[c + 1], of which the first
 * class_len[c] are live and the rest is padding (allocated and loaded, but its content, NaN included, never reaches out).
 * class_off int32 [C + 1] and class_len int32 [C] are DEVICE arrays with: class_off[0] == 0, every class_off[c] a multiple
 * of 16, ascending, class_off[C] == Np, 0 <= class_len[c] <= class_off[c + 1] - class_off[c].  The entry cannot see their
 * content without a host read, so that part of the contract is the caller's to check (cclip_hip/ops.py does, on the host
 * copies it uploads); the kernels clamp every cursor they derive from the two arrays, so no content makes them read or
 * write out of bounds.  exclude: int32 [Q] on the device, a row of g to leave out per query (-1: none), or NULL.
 * An empty class gives exactly 0.0f, and so does a class whose only live row is excluded.  The Q x Np matrix is never
 * written.  The stored rows are split by a rule that depends on Np alone and every sum runs in a fixed order without
 * atomics: two launches are bitwise equal, and a query's row of out does not depend on Q or on the other queries.
 * Two launches on `stream`: per-split class sums into `workspace`, then the merge.  workspace: at least
 * cclip_cache_affinity_workspace(Q, Np, C) = Q * splits(Np) * C * 4 bytes (0 for arguments the call would refuse; splits(Np)
 * <= min(512, ceil(Np / 256))), 4-byte aligned device memory the caller owns; its contents before and after are meaningless.
 * Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched, out untouched): null q, g, class_off, class_len, out or workspace; Q <= 0; Np <= 0,
 * Np >= 2^31 or Np % 16; C < 1 or C > 256; D < 32, D % 32 or D > 1024; ldq or ldg below D or not a multiple of 8; q or g not
 * 16-byte aligned; a misaligned int32 / fp32 array; workspace too small. */
int64_t cclip_cache_affinity_workspace(int32_t Q, int64_t Np, int32_t C);
int cclip_cache_affinity(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t Np, int32_t D,
                         const int32_t* class_off, const int32_t* class_len, int32_t C, float beta, const int32_t* exclude,
                         float* out, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- gradient of the class affinities with respect to the stored rows (csrc/embed_cache_bwd.hip) -------------------
 * Operands, layout contract and limits of cclip_cache_affinity; dA fp32 [Q, C] contiguous, dG fp32 [Np, D] contiguous and
 * 16-byte aligned.  With s as above and c(n) the class whose segment holds row n:
 *   dG[n, :] = beta * sum over the queries i with n != exclude[i] of dA[i, c(n)] * exp(beta * (s[i, n] - 1)) * q[i, :]   live rows n
 *   dG[n, :] = +0.0f                                                                                         padding rows n
 * Every row of dG is written; the content of the padding rows of g, NaN included, never reaches it.  The Q x Np matrix is
 * never written.  The weights dA * exp(..) enter the second MFMA product as a 16-bit hi + lo pair after a power-of-two scale
 * taken from max|dA| on the device (relative error 2^-16 per term in bf16, 2^-22 in fp16).  No atomics, one fixed order:
 * two launches are bitwise equal.  Two launches on `stream`: the partial maxima of |dA| into `workspace`, then the gradient.
 * workspace: at least cclip_cache_affinity_bwd_workspace(Q, C) = 256 bytes (0 for arguments the call would refuse), 4-byte
 * aligned device memory the caller owns.  Nothing is read on the host.  The kernels clamp every cursor they derive from
 * class_off / class_len: no content makes them read or write out of bounds.
 * CCLIP_ERR_ARG (nothing launched, dG untouched): the cases of cclip_cache_affinity; null dA or dG; dG not 16-byte aligned. */
int64_t cclip_cache_affinity_bwd_workspace(int32_t Q, int32_t C);
int cclip_cache_affinity_bwd(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t Np, int32_t D,
                             const int32_t* class_off, const int32_t* class_len, int32_t C, float beta, const int32_t* exclude,
                             const float* dA, float* dG, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- spherical k-means over stored embeddings: the assignment step (csrc/embed_kmeans.hip) ----------------------------
 * For rows x [N, D] and centroids c [K, D], both bf16 (fp16 in the twin) with row strides ldx / ldc in elements and inner
 * stride 1, with s[n, k] = sum_d x[n, d] c[k, d] accumulated in fp32 on the MFMA (one chain over d = 0, 32, ..: the score
 * bits cclip_similarity_topk returns for the pair):
 *   assign[n] int32: the centroid with the largest s[n, .]        best[n] fp32: that score
 *   second[n] fp32 (may be NULL): the second-largest score of the row, NaN if K == 1
 * Order as in cclip_similarity_topk: equal fp32 scores (-0 == +0) go to the LOWER centroid index, a NaN score ranks below
 * every number (a row whose scores are all NaN gets centroid 0 and best = NaN).  (assign, best, second) are the first two
 * entries cclip_similarity_topk(x, c, min(2, K)) returns, bit for bit.  The N x K matrix is never written and there is no
 * workspace: one launch on `stream` whose grid runs over blocks of rows while all K centroids stream through LDS.  No
 * atomics: two launches are bitwise equal, and a row's outputs do not depend on N or on the other rows.  Nothing is read on
 * the host.
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): null x, c, assign or best; N <= 0 or N >= 2^31; K <= 0 or K >= 2^31;
 * D < 32, D % 32 or D > 1024; ldx or ldc below D or not a multiple of 8; x or c not 16-byte aligned; a misaligned output. */
int cclip_kmeans_assign(const void* x, int64_t ldx, int64_t N, const void* c, int64_t ldc, int64_t K, int32_t D,
                        int32_t* assign, float* best, float* second, hipStream_t stream);

/* ---- spherical k-means: the centroid step (csrc/embed_kmeans.hip) ---------------------------------------------------
 * x as above.  order int32 [N] and seg_off int32 [K + 1] are DEVICE arrays: order lists the rows of x grouped by cluster,
 * ascending row index inside a cluster, and cluster k owns the positions seg_off[k] .. seg_off[k + 1] of it (seg_off[0] == 0,
 * ascending, seg_off[K] == N).  For cluster k with S = the sum of its rows in fp32:
 *   out_norm[k] = |S|_2  fp32 [K]        out_c[k, :] = S / |S|, rounded once to the 16-bit type   [K, D], row stride ldo
 * An empty cluster, and one whose |S| is 0 or not finite, gets prev_c[k, :] (row stride ldp) bit for bit and out_norm[k] = 0;
 * out_c may be prev_c itself.  The sums run in one fixed order that depends on (N, D, order, seg_off) alone - slabs of 256
 * positions of `order`, no atomics, no fused multiply-add: the outputs are a pure function of (x, order, seg_off, prev_c) and
 * two launches are bitwise equal.  A lopsided clustering costs what a balanced one costs.
 * The entry cannot see the content of order / seg_off without a host read, so that they are a permutation and its monotone
 * boundaries is the caller's to ensure (cclip_hip/ops.py builds both with a stable sort); the kernels clamp every value they
 * take from the two arrays, so no content makes them read or write outside x, the workspace or the outputs.
 * Two launches on `stream`: per-slab partial sums into `workspace`, then one work-group per cluster.  workspace: at least
 * cclip_kmeans_update_workspace(N, K, D) = (ceil(N / 256) + K) * D * 4 bytes (0 for arguments the call would refuse), 4-byte
 * aligned device memory the caller owns; its contents before and after are meaningless.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): a null pointer; N <= 0 or N >= 2^31; K <= 0 or K >= 2^31; D < 32,
 * D % 32 or D > 1024; ldx below D or not a multiple of 8; x not 16-byte aligned; ldp or ldo below D; a misaligned int32 /
 * fp32 / 16-bit array; workspace too small. */
int64_t cclip_kmeans_update_workspace(int64_t N, int64_t K, int32_t D);
int cclip_kmeans_update(const void* x, int64_t ldx, int64_t N, int32_t D, const int32_t* order, const int32_t* seg_off,
                        int64_t K, const void* prev_c, int64_t ldp, void* out_c, int64_t ldo, float* out_norm,
                        void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- coreset selection: one k-centre greedy pick per launch (csrc/coreset.hip) ------------------------------------------
 * State, all on the device: x [N, D] unit bf16 rows (fp16 in the twin) under the contract of cclip_kmeans_assign (row stride
 * ldx in elements, inner stride 1, 16-byte aligned); weight fp32 [N] or NULL (= 1); mind fp32 [N], the row's cosine distance
 * 1 - <x_i, x_c> to its nearest centre so far, +inf = none yet; owner int32 [N], that centre's row, -1 = none, owner[i] == i
 * marks a row that is itself a centre; partial_in / partial_out, two DIFFERENT buffers of P = cclip_coreset_blocks(N) 64-bit
 * keys each (8-byte aligned).  A key holds the order-preserving image of weight[i] * mind[i] in the high word and ~i in the
 * low one.  Order as in cclip_similarity_topk: larger = better, equal fp32 values (-0 == +0) go to the LOWER row, a NaN value
 * ranks below every number; key 0 = no eligible row.  A row is eligible if owner[i] != i and its weight, where given, is > 0
 * (a NaN weight is not); its value may be +inf.
 * `centre` picks the mode:
 *   centre >= 0                        that row is the centre c (the first pick without seeds); partial_in is not read
 *   CCLIP_CORESET_FROM_PARTIALS (-1)   c = the row of the largest of the P keys of partial_in, clamped into [0, N - 1] before
 *                                      use.  All keys 0: pick_out[0] = -1, radius_out[0] = NaN, mind and owner untouched.
 *   CCLIP_CORESET_SCAN_ONLY (-2)       no centre and no update (after seeding); pick_out / radius_out are not written
 * With a centre: pick_out[0] = c and radius_out[0] = mind[c] as it was BEFORE this launch (the covering radius of everything
 * chosen before this pick), then mind[c] = 0, owner[c] = c; every other row that is not a centre with d = 1 - s < mind[i]
 * takes mind[i] = d, owner[i] = c - strictly smaller, so an equal distance keeps the earlier centre, and a NaN d changes
 * nothing.  In every mode partial_out[b] then receives the best key among the eligible rows of work-group b (0 if none).
 * The dot.  s is ONE fixed fp32 order that depends on D alone: a row belongs to a team of T lanes, T = the power of two
 * >= D / 8 capped at 64; lane l adds the exact products of elements 8 l .. 8 l + 7 in ascending order from the first, for
 * D > 512 the products of elements 512 + 8 l .. likewise and that sum to the first; the team then adds by an xor butterfly
 * over lane distances 1, 2, .. T / 2.  No fused multiply-add.  A row's new mind and owner are a function of (x_i, x_c, old
 * mind, old owner) alone - not of N, of the row's position or of the grid.
 * One launch of cclip_coreset_blocks(N) = min(1024, ceil(N / 64)) work-groups (0 for an N the call would refuse), rows dealt
 * by a grid stride.  The work-groups agree on c without talking, because the maximum of distinct keys has no order: no
 * atomics, no spin-wait, no cross-work-group barrier; two launches are bitwise equal.  c is the only index taken from device
 * memory.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): null x, mind, owner or partial_out; N <= 0 or N >= 2^31; D < 32, D % 32
 * or D > 1024; ldx below D or not a multiple of 8; x not 16-byte aligned; centre < -2 or >= N; null partial_in with
 * CCLIP_CORESET_FROM_PARTIALS; partial_in == partial_out; null pick_out or radius_out unless CCLIP_CORESET_SCAN_ONLY; a
 * misaligned fp32 / int32 array or a partial buffer not 8-byte aligned. */
#define CCLIP_CORESET_FROM_PARTIALS (-1)
#define CCLIP_CORESET_SCAN_ONLY (-2)
int32_t cclip_coreset_blocks(int64_t N);
int cclip_coreset_step(const void* x, int64_t ldx, int64_t N, int32_t D, const float* weight, float* mind, int32_t* owner,
                       int32_t centre, const void* partial_in, void* partial_out, int32_t* pick_out, float* radius_out,
                       hipStream_t stream);

/* ---- coreset selection: m picks from one call (csrc/coreset.hip) -----------------------------------------------------------
 * The m launches of cclip_coreset_step enqueued from one C loop: pick t reads the keys of partial[t & 1] and writes
 * partial[(t + 1) & 1], partial[j] = workspace + j * P keys; picks int32 [m] and radius fp32 [m] receive pick_out /
 * radius_out of launch t at position t.  first >= 0: launch 0 takes that row as its centre; first ==
 * CCLIP_CORESET_FROM_PARTIALS: partial[0] already holds the keys of the state (a CCLIP_CORESET_SCAN_ONLY step into it, or
 * partial_out of an earlier pick).  The outputs and the state equal those of m single steps bit for bit; after the call the
 * keys of the state are in partial[m & 1].  Once no eligible row is left the remaining picks are -1 with radius NaN.  m == 0
 * launches nothing.  workspace: at least cclip_coreset_workspace(N) = 2 * cclip_coreset_blocks(N) * 8 bytes (0 for an N the
 * call would refuse), 8-byte aligned device memory the caller owns.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): the cases of cclip_coreset_step for x, ldx, N, D, weight, mind and
 * owner; m < 0 or m > N; first < -1 or >= N; null, misaligned or too small workspace; null picks or radius with m > 0; a
 * misaligned picks or radius. */
int64_t cclip_coreset_workspace(int64_t N);
int cclip_coreset_greedy(const void* x, int64_t ldx, int64_t N, int32_t D, const float* weight, float* mind, int32_t* owner,
                         int32_t first, int64_t m, int32_t* picks, float* radius, void* workspace, int64_t workspace_bytes,
                         hipStream_t stream);

/* ---- mutual-reachability nearest row outside the own component (csrc/mst.hip) -------------------------------------------
 * x [N, D] unit bf16 rows (fp16 in the twin) under the contract of cclip_kmeans_assign (row stride ldx in elements, inner
 * stride 1, 16-byte aligned); core fp32 [N]; comp int32 [N]; keys 64-bit [N], 8-byte aligned.  With s[i, j] the fp32 MFMA
 * score (one chain over d = 0, 32, ..: the bits cclip_similarity_topk returns for the pair) and
 *   m[i, j] = min(s[i, j], core[i], core[j])     taken on the order images: -0 == +0, a NaN operand gives NaN, the lowest
 * keys[i] = the largest key over the rows j with comp[j] != comp[i], a key being the order image of m in the high word and ~j
 * in the low one: larger m first, equal m to the LOWER j (the order of cclip_similarity_topk); 0 = no such row.  comp is
 * only compared, never used as an index: any int32 value is legal.  core = +inf leaves the plain similarity.
 * The N x N matrix is never written.  The grid runs over blocks of rows x cclip_mreach_nearest_splits(N) gallery splits; with
 * more than one split keys is zeroed on `stream` first and the splits meet in a 64-bit integer atomicMax, whose result has
 * no order: the output is a pure function of (x, core, comp), two launches are bitwise equal.  No workspace, no float
 * atomics, nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched, keys untouched): null x, core, comp or keys; N <= 0 or N >= 2^31; D < 32, D % 32 or
 * D > 1024; ldx below D or not a multiple of 8; x not 16-byte aligned; a misaligned core, comp or keys. */
int32_t cclip_mreach_nearest_splits(int64_t N);
int cclip_mreach_nearest(const void* x, int64_t ldx, int64_t N, int32_t D, const float* core, const int32_t* comp, void* keys,
                         hipStream_t stream);

/* ---- maximum spanning tree under mutual-reachability similarity: Boruvka, one call (csrc/mst.hip) ------------------------
 * x, core as above.  The tree is the maximum spanning tree of the complete graph on the rows under the strict total order
 *   {i, j} before {k, l}:  larger m (order images);  equal m: smaller min(i, j);  then smaller max(i, j)
 * which is unique - a pure function of the score bits and core, not of the grid, the splits or the launch order.
 * u, v int32 [N], m fp32 [N]: N - 1 slots hold an edge (u[k] != v[k], both in [0, N), m[k] = m[u[k], v[k]]) and exactly one
 * slot holds u = v = -1, m = NaN.  Which slot an edge lands in is fixed too (the name of the component that chose it).
 * ceil(log2 N) rounds are enqueued from one C loop: the nearest kernel above, two integer-atomic reductions to every
 * component's best outgoing edge, the hooks, the relabelling.  A device flag marks "one component left"; the kernels of
 * later rounds return at once.  Rounds alternate between two label buffers.  Every index a kernel takes from memory is
 * clamped.  Nothing is read on the host; N == 1 only writes the empty slot.
 * workspace: at least cclip_mst_workspace(N) = 32 N + 256 bytes (0 for an N the call would refuse), 8-byte aligned device
 * memory the caller owns; its contents before and after are meaningless.
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): the cases of cclip_mreach_nearest for x, ldx, N, D and core; null or
 * misaligned u, v or m; null, misaligned or too small workspace. */
int64_t cclip_mst_workspace(int64_t N);
int cclip_mst_boruvka(const void* x, int64_t ldx, int64_t N, int32_t D, const float* core, int32_t* u, int32_t* v, float* m,
                      void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- linear probe: logistic regression on stored embeddings (csrc/embed_probe.hip) -------------------------------------
 * x [N, D] bf16 (fp16 in the twin), row stride ldx in elements, inner stride 1; W fp32 [C, D] contiguous; bias fp32 [C] or NULL
 * (= 0); labels int32 [N] or NULL (= every row ignored), a label < 0 or >= C means the row is ignored; row_weight fp32 [N] or
 * NULL (= 1), clamped into [0, 1] by the kernel, NaN -> 0.  2 <= C <= 256, 32 <= D <= 1024, D % 32 == 0, N < 2^31.
 * THE OBJECTIVE OF hi + lo.  W enters the MFMA as the 16-bit pair hi = round16(W), lo = round16(W - hi), written by a small
 * launch into the workspace, and both entries compute functions of that pair:
 *   z[n, c]   = (bias[c] + H[n, c]) + L[n, c], H = sum_d x[n, d] hi[c, d], L = sum_d x[n, d] lo[c, d]: each ONE fp32 accumulator
 *               chain over d = 0, 32, .. on the MFMA, the two adds in the order written
 *   rw[n]     = the clamped row_weight;  live(n) = 0 <= labels[n] < C and rw[n] > 0
 * cclip_probe_forward, per row (all [N] contiguous; a row's outputs depend on neither N nor the row's position):
 *   lse[n]    = log sum_c exp z[n, c], by a running maximum (logits of the order of 100 do not overflow)
 *   loss[n]   = rw[n] (lse[n] - z[n, labels[n]]) for a live row, exactly +0.0f otherwise - SELECTED, never multiplied: an
 *               ignored row of NaN leaves no trace
 *   pred[n]   = argmax_c z[n, c] int32: equal fp32 logits (-0 == +0) go to the LOWER class, a NaN logit ranks below every number
 *   logits    = NULL, or fp32 [N, C] contiguous that receives z; the N x C matrix is written in no other case
 * cclip_probe_backward takes the forward's lse (and loss, for the objective) of the SAME operands:
 *   g[n, c]   = rw[n] (exp(z[n, c] - lse[n]) - [c == labels[n]]) for a live row, 0 otherwise (selected); |g| <= 1, and g enters
 *               the second MFMA product as a 16-bit hi + lo pair (what is dropped: 2^-16 relative in bf16, 2^-22 in fp16, plus
 *               2^-25 absolute in fp16)
 *   dW[c, :]  = scale * sum_n g[n, c] x[n, :] + l2 * W[c, :]   fp32 [C, D]        db[c] = scale * sum_n g[n, c]   fp32 [C]
 *   objective = scale * sum_n loss[n] + l2 / 2 * sum W^2   fp32 [1]; loss and objective are both given or both NULL
 * dW is the gradient of the objective as a function of the pair (hi + lo differs from W by less than 2^-16 |W| in bf16,
 * 2^-22 |W| in fp16): loss and gradient belong to one function.  The bias is not regularised.  `scale` is the caller's
 * 1 / (sum of the live rows' weights).
 * Order.  The rows are split over the grid in parts of cclip_probe_parts-many slots: a wave adds its row tiles of 32 in
 * ascending order in registers and writes one fp32 partial per slot; the merge adds the slots in ascending order; loss and W^2
 * are reduced by a fixed tree.  The slot count and every other choice depend on (N, C, D) alone, there are no atomics and no
 * fused multiply-add: two calls are bitwise equal.  Every value taken from labels is compared, never used as an address.
 * Launches on `stream`: forward 2 (pair image, rows); backward 3, or 4 with the objective (pair image, partials, merge,
 * objective).  Nothing is read on the host.
 * workspace: at least cclip_probe_workspace(N, C, D) bytes for either entry (0 for arguments they would refuse), 16-byte
 * aligned device memory the caller owns, contents meaningless before and after.  With Cp = 16 ceil(C / 16),
 * rs = 4, 2, 1 for Cp = 16, 32, >= 48, T = ceil(N / 32), Pmax = clamp(2^25 / (4 rs Cp D), 1, 1024), tpp = max(8, ceil(T / Pmax))
 * and S = rs ceil(T / tpp) = cclip_probe_parts(N, C, D):
 *   bytes = 4 Cp D  (the pair image)  +  4 S Cp (D + 1)  (the partials of dW and db, at most 32 MB + 4 S Cp)
 *         + 4 (ceil(C D / 256) + 256)  (the reduction tree)
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): null x, W or workspace; forward: null lse, loss or pred; backward: null
 * lse, dW or db, loss without objective or objective without loss, scale or l2 negative or not finite; N <= 0 or N >= 2^31;
 * C < 2 or C > 256; D < 32, D % 32 or D > 1024; ldx below D or not a multiple of 8; x or workspace not 16-byte aligned; a
 * misaligned int32 / fp32 array; workspace too small. */
int64_t cclip_probe_workspace(int64_t N, int32_t C, int32_t D);
int32_t cclip_probe_parts(int64_t N, int32_t C, int32_t D);
int cclip_probe_forward(const void* x, int64_t ldx, int64_t N, int32_t D, const float* W, const float* bias, int32_t C,
                        const int32_t* labels, const float* row_weight, float* lse, float* loss, int32_t* pred, float* logits,
                        void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_probe_backward(const void* x, int64_t ldx, int64_t N, int32_t D, const float* W, const float* bias, int32_t C,
                         const int32_t* labels, const float* row_weight, const float* lse, const float* loss, float scale,
                         float l2, float* dW, float* db, float* objective, void* workspace, int64_t workspace_bytes,
                         hipStream_t stream);

/* ---- Concept decomposition: sparse non-negative codes over a dictionary (csrc/concept_codes.hip) -------------------------
 * x [N, D] and the dictionary c [V, D]: unit bf16 rows (fp16 in the twin) under the contract of cclip_kmeans_assign (row
 * strides ldx, ldc in elements, multiples of 8, 16-byte aligned).  Per row of x, independently,
 *   minimise over w >= 0:  1/2 |x - sum_v w_v c_v|^2 + l1 sum_v w_v
 * by exactly `iters` FISTA iterations with the non-negative soft threshold, step eta (the caller's 1 / L, L the largest
 * eigenvalue of c^T c; never computed here) and beta_k = k / (k + 3), w_0 = w_{-1} = 0:
 *   y_k = w_k + beta_k (w_k - w_{k-1});   g_v = <c_v, x - sum_u y_{k,u} c_u>;   w_{k+1,v} = max(0, y_{k,v} + eta (g_v - l1))
 * in fp32.  The residual x - sum y c is carried in fp32 at the point the next gradient is taken at (y_{k+1}; w_T in the last
 * iteration) and enters the MFMA, as the tile of y does, as the 16-bit pair hi = round16(v), lo = round16(v - hi) (what is
 * dropped: 2^-16 relative in bf16, 2^-22 in fp16).  A padding concept (V up to the tile of 32) counts as a zero row: its weight
 * is never written and never counted.
 * Outputs: w fp32 [N, V] (row stride ldw >= V elements, a multiple of 4, 16-byte aligned; nothing is written between the rows)
 * = w_T, and per row, from a closing sweep at w_T itself (each [N] contiguous):
 *   resid2 = |x - sum w c|^2   l1norm = sum w   nnz = #{w > 0} int32   delta = max_v |w_T - w_{T-1}|
 *   kkt    = max_v (w_v > 0 ? |g_v - l1| : max(0, g_v - l1)): the row's distance from optimality
 * iters == 0 gives w = 0, resid2 = |x|^2, delta = 0.  A row of x that holds a NaN gets NaN weights and NaN float read-outs
 * (nnz 0) for iters >= 1 and touches no other row.  A row's outputs are a function of (the row, c, l1, eta, iters) alone - not
 * of N, the row's position or the grid; no atomics, no fused multiply-add, one summation order: two calls are bitwise equal.
 * ONE launch on `stream` runs every iteration (a work-group owns 32 rows at D <= 512, 16 above, and re-streams c per
 * iteration); nothing is read on the host.
 * workspace: at least cclip_concept_codes_workspace(N, V, D) = 4 N * 4 ceil(V / 4) bytes (0 for arguments the call would
 * refuse), 16-byte aligned: w_{k-1}.  Contents meaningless before and after.
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): a null pointer; N <= 0 or N >= 2^31; V < 1 or V > 2^24; D < 32, D % 32
 * or D > 1024; ldx or ldc below D or not a multiple of 8, x or c not 16-byte aligned; ldw below V or not a multiple of 4, w or
 * workspace not 16-byte aligned; a misaligned read-out array; l1 or eta negative or not finite; iters < 0; workspace too
 * small. */
int64_t cclip_concept_codes_workspace(int64_t N, int64_t V, int32_t D);
int cclip_concept_codes(const void* x, int64_t ldx, int64_t N, const void* c, int64_t ldc, int64_t V, int32_t D, float l1,
                        float eta, int32_t iters, float* w, int64_t ldw, float* resid2, float* l1norm, int32_t* nnz,
                        float* delta, float* kkt, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- Gaussian class models: second moments of stored embeddings (csrc/embed_moments.hip) ---------------------------------
 * x [N, D] bf16 (fp16 in the twin) under the contract of cclip_kmeans_assign (row stride ldx in elements, a multiple of 8, inner
 * stride 1, 16-byte aligned; D % 32 == 0, 32 <= D <= 1024, N < 2^31); labels int32 [N], or NULL with C == 1 (every row is class
 * 0); 1 <= C <= 256.  A row whose label lies outside [0, C) is dropped from every output.
 *   count int32 [C] = rows per class     sum fp32 [C, D] = sum of the class's rows     gram fp32 [D, D] = sum_live x^T x
 * Products of two 16-bit values are exact in fp32 and enter one fp32 accumulator chain per entry and part on the MFMA, rows in
 * ascending order (both products are [onehot(labels) | x]^T x over tiles of 32 rows).  The rows are split into
 * cclip_moments_parts(N, C, D) parts of tpp consecutive tiles; a second launch adds the parts in a fixed tree (runs of 8 in
 * ascending order, the runs in ascending order) and writes gram[a, b] and gram[b, a] from the same value: gram is bitwise
 * symmetric, only block pairs on and above the diagonal are computed.  Padding rows and dropped rows add exactly +0.  A NaN or
 * Inf in column a of a live row of class c reaches row and column a of gram (its outer product: NaN * 0 is NaN) and sum[c, a],
 * and nothing else: in the one-hot product such an element enters as zero and is recorded by an integer atomic OR, from which
 * the merge restores NaN / +Inf / -Inf.  count is added by integer atomics.  No float atomics; every choice is a function of
 * (N, C, D) alone; two calls are bitwise equal.  Three launches on `stream`; nothing is read on the host.
 * workspace: at least cclip_moments_workspace(N, C, D) bytes (0 for arguments the call would refuse), 16-byte aligned, contents
 * meaningless before and after.  With B = ceil(D / 128), J = B (B + 1) / 2 + ceil(C / 128) B jobs of one 128 x 128 block each,
 * T = ceil(N / 32), Pmax = clamp(2^25 / (65536 J), 1, 1024), tpp = max(8, ceil(T / Pmax)), P = ceil(T / tpp) = cclip_moments_parts:
 *   bytes = 65536 P J  (the partial blocks, at most 32 MB)  +  4 C D  (the flags)
 * CCLIP_ERR_ARG (nothing launched, outputs untouched): a null x, count, sum, gram or workspace; labels NULL with C != 1;
 * N <= 0 or N >= 2^31; C < 1 or C > 256; D < 32, D % 32 or D > 1024; ldx below D or not a multiple of 8; x or workspace not
 * 16-byte aligned; a misaligned int32 / fp32 array; workspace too small. */
int64_t cclip_moments_workspace(int64_t N, int32_t C, int32_t D);
int32_t cclip_moments_parts(int64_t N, int32_t C, int32_t D);
int cclip_class_moments(const void* x, int64_t ldx, int64_t N, int32_t D, const int32_t* labels, int32_t C, int32_t* count,
                        float* sum, float* gram, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- Gaussian class models: transform, distances to centres, scores (csrc/gauss_scores.hip) -------------------------------
 * x [Q, D] 16-bit under the contract above; T fp32 [R, D] contiguous, 1 <= R <= 1024 (padded to 16 inside); t0 fp32 [R] or
 * NULL (= 0); centres fp32 [C, R] contiguous with 1 <= C <= 256, or NULL with C == 0; offset fp32 [C] or NULL (= 0).
 * T enters the MFMA as the 16-bit pair hi = round16(T), lo = round16(T - hi) - the pair of W in cclip_probe_forward - written
 * by a small launch into the workspace:
 *   z[q, r]     = acc - t0[r]; acc is ONE fp32 accumulator chain that takes x * hi, then x * lo, of every k-step d = 0, 32, ..
 *   d2[q, c]    = sum_r (z[q, r] - centres[c, r])^2   fp32, r ascending; subtract, multiply, add - the expansion
 *                 |z|^2 - 2 z.m + |m|^2 is NOT used: it cancels once T is an ill-conditioned whitening
 *   score[q, c] = -0.5 d2[q, c] + offset[c]
 * Per row (each [Q] contiguous): pred int32 = argmax_c score (equal scores go to the LOWER class, NaN ranks lowest);
 * lse fp32 = log sum_c exp score by a running maximum; nearest int32 = argmax_c (-d2) under the same rule; dmin = d2[q, nearest].
 * d2 fp32 [Q, C] and z fp32 [Q, R] are written only where the pointer is not NULL.  With centres == NULL only z is written
 * (required then; offset and d2 must be NULL): the PCA transform.  A work-group keeps its rows' z in LDS between the stages.
 * A row's outputs depend on neither Q nor its position; a row with a NaN gets NaN z, d2, lse and dmin, pred = nearest = 0, and
 * touches no other row.  No atomics, no fused multiply-add; two calls are bitwise equal.  Two launches; no host read.
 * workspace: at least cclip_gauss_scores_workspace(R, D) = 4 * 16 ceil(R / 16) * D bytes (the pair image; 0 for sizes the call
 * would refuse), 16-byte aligned.
 * CCLIP_ERR_ARG (nothing launched): a null x, T or workspace; centres without pred, lse, nearest or dmin, or C outside 1 .. 256;
 * no centres and no z, or offset, d2 or C != 0 without centres; Q <= 0 or Q >= 2^31; R < 1 or R > 1024; D < 32, D % 32 or
 * D > 1024; ldx below D or not a multiple of 8; x or workspace not 16-byte aligned; a misaligned array; workspace too small. */
int64_t cclip_gauss_scores_workspace(int64_t R, int32_t D);
int cclip_gauss_scores(const void* x, int64_t ldx, int64_t Q, int32_t D, const float* T, const float* t0, int32_t R,
                       const float* centres, const float* offset, int32_t C, int32_t* pred, float* lse, int32_t* nearest,
                       float* dmin, float* d2, float* z, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- t-SNE of stored embeddings: neighbour probabilities (csrc/tsne.hip, fp32 only) -------------------------------------
 * scores fp32 [N, k] (row stride ld >= k elements): the similarities of every row's k nearest OTHER unit rows, in any order.
 * Per row, with d2_j = 2 - 2 s_j (a negative value taken as 0) and diff_j = d2_j - min_j d2_j, all in fp32:
 *   p_j ~ exp(-beta diff_j), normalised;   H(beta) = log sum_j e_j + beta sum_j diff_j e_j / sum_j e_j   (nats)
 * beta is found by exactly 100 entropy evaluations and no data-dependent exit: beta = 1, lo = 0, no upper bound; H > log
 * perplexity sets lo = beta, then beta = (lo + hi) / 2 if an upper bound is known, else 2 beta; otherwise hi = beta and
 * beta = (lo + hi) / 2.  The beta after the last step is written, and P from it:
 *   P fp32 [N, k] contiguous, every row summing to 1 within k 2^-24;   beta fp32 [N]
 * A row whose k distances are equal gets P = 1 / k (beta ends as 2^100); where the m >= perplexity smallest distances are
 * equal the target cannot be met and P tends to 1 / m on them.  d2 = 0 is legal.  A NaN score makes its row's P and beta NaN
 * and touches no other row.  One launch, one thread per row, no workspace; nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): a null or misaligned pointer; N <= 0 or N >= 2^31; k < 1 or k > 63; ld < k; perplexity
 * not inside (1, k). */
int cclip_tsne_affinities(const float* scores, int64_t ld, int64_t N, int32_t k, float perplexity, float* P, float* beta,
                          hipStream_t stream);

/* ---- t-SNE: the N-body sums (csrc/tsne.hip) ----------------------------------------------------------------------------
 * y fp32 [N, 2] contiguous.  With w_ij = 1 / (1 + |y_i - y_j|^2), over ALL j != i (the diagonal adds nothing, to Z included;
 * a coincident point j != i adds 1 to zrow and 0 to rep):
 *   zrow[i] = sum_j w_ij  fp32 [N]      rep[i, :] = sum_j w_ij^2 (y_i - y_j)  fp32 [N, 2]      z_sum[0] = sum_i zrow[i]
 * Order.  Work-groups of 256 rows stream y through LDS in tiles of 512 points; the j range is cut into
 * cclip_tsne_repulsion_splits(N) <= 16 runs of whole tiles (enough that N = 20 000 fills the machine).  Inside a split four
 * chains take j = 0, 1, 2, 3 mod 4 of every tile (the last j mod 4 points of a short tile join chain 0) and are added
 * (c0 + c1) + (c2 + c3); a row's splits are added in ascending order; z_sum is a fixed tree over blocks of 256 rows.  1 / x
 * is v_rcp_f32 (1 ulp).  No atomics, every choice a function of N alone: two calls on the same y are bitwise equal.
 * Three launches on `stream`; nothing is read on the host.  workspace: at least cclip_tsne_repulsion_workspace(N) =
 * (3 N splits + ceil(N / 256)) * 4 bytes (0 for an N the call would refuse), 4-byte aligned, contents meaningless.
 * CCLIP_ERR_ARG (nothing launched): a null pointer; N <= 0 or N >= 2^31; y or rep not 8-byte aligned, another pointer not
 * 4-byte aligned; workspace too small. */
int32_t cclip_tsne_repulsion_splits(int64_t N);
int64_t cclip_tsne_repulsion_workspace(int64_t N);
int cclip_tsne_repulsion(const float* y, int64_t N, float* zrow, float* rep, float* z_sum, void* workspace,
                         int64_t workspace_bytes, hipStream_t stream);

/* ---- t-SNE: one gradient-descent update (csrc/tsne.hip) ----------------------------------------------------------------
 * y, vel, gains, rep, y_out fp32 [N, 2] contiguous; the symmetric joint probabilities as CSR: offsets int64 [N + 1], cols
 * int32 [nnz], vals fp32 [nnz] (an empty row is legal); z_sum the device scalar of cclip_tsne_repulsion for the same y.
 * Per row i, its entries in ascending position, q_ij = 1 + |y_i - y_j|^2:
 *   att_i  = sum_j (exaggeration P_ij / q_ij) (y_i - y_j)            grad_i = 4 (att_i - rep_i / Z)
 *   gains  : + 0.2 where (vel > 0) != (grad > 0), else * 0.8; then max(gains, min_gain)       (in place)
 *   vel    = momentum vel - learning_rate gains grad                                           (in place)
 *   y_out  = y + vel      - a SECOND buffer: other rows still read y
 *   kl_row[i] = sum_j P_ij ((log P_ij + log q_ij) + log Z) over the entries with P_ij > 0, P NOT exaggerated   (may be NULL)
 * With y_out NULL only kl_row is written (vel, gains and rep are not touched and may be NULL).  One launch, one thread per
 * row, no atomics: bitwise repeatable.  offsets and cols are clamped before use, so no content makes the kernel leave its
 * arrays.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): null y, offsets or z_sum; null cols / vals with nnz > 0; y_out and kl_row both null;
 * y_out given with a null vel, gains or rep, or y_out == y; N <= 0 or N >= 2^31; nnz < 0; a misaligned pointer. */
int cclip_tsne_step(const float* y, float* vel, float* gains, int64_t N, const int64_t* offsets, const int32_t* cols,
                    const float* vals, int64_t nnz, const float* rep, const float* z_sum, float exaggeration, float momentum,
                    float learning_rate, float min_gain, float* y_out, float* kl_row, hipStream_t stream);

/* ---- label spreading: the normalised graph operator (csrc/label_spread.hip, fp32 only) -----------------------------------
 * A symmetric non-negative graph W as CSR: offsets int64 [N + 1], cols int32 [nnz], vals fp32 [nnz]; an empty row is legal.
 *   deg[i]      = d_i, the sum of row i's entries in ascending position                                   fp32 [N]
 *   r_i         = 1.0f / sqrtf(d_i), and 0 where d_i is not > 0 (an empty row, a row of zero weights, a NaN)
 *   vals_out[e] = (vals[e] * r_i) * r_j  for the entry e of row i with column j: D^-1/2 W D^-1/2           fp32 [nnz]
 * A row of zero weights gives zeros, never NaN or inf.  vals_out == vals is legal.  offsets are clamped into [0, nnz] and
 * made non-decreasing per row, cols into [0, N - 1], before use: no content makes a kernel leave its arrays (rows that such
 * offsets make overlap are written once per row, in no defined order).  Two launches, one thread per row, no atomics:
 * bitwise repeatable.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): null offsets or deg; null cols, vals or vals_out with nnz > 0; N <= 0, N or nnz >= 2^31,
 * nnz < 0; a misaligned pointer. */
int cclip_label_graph_normalize(const int64_t* offsets, const int32_t* cols, const float* vals, int64_t N, int64_t nnz,
                                float* deg, float* vals_out, hipStream_t stream);

/* ---- label spreading: one iteration (csrc/label_spread.hip) --------------------------------------------------------------
 * F_in, F_out fp32 [N, C] contiguous, S as CSR (the vals_out above), labels int32 [N], class_weight fp32 [C] or NULL:
 *   F_out[i, c]  = alpha * sum_j S_ij F_in[j, c] + (1 - alpha) * y_ic
 *   y_ic         = (class_weight ? class_weight[c] : 1) where labels[i] == c, else 0
 *   delta_row[i] = max_c |F_out[i, c] - F_in[i, c]|   (may be NULL; NaN if any of the row's differences is)     fp32 [N]
 * labels[i] < 0 marks an unlabelled row; labels[i] >= C is taken as unlabelled too and indexes nothing.
 * Order.  A row belongs to a team of G * CW lanes, CW = the power of two >= min(C, 64), G = cclip_label_spread_groups(C) =
 * min(8, 64 / CW); 256 / (G CW) rows share a work-group.  Edge group g adds the row's entries at positions g, g + G, .. in
 * ascending order as one fma chain from 0; the G chains are added in the tree ((g0 + g1) + (g2 + g3)) + ((g4 + g5) +
 * (g6 + g7)).  For C > 64 a lane holds 2 (C <= 128) or 4 classes, 64 apart, and C > 256 takes one pass over the row per 256
 * classes.  The label term is fma(-alpha, w, w), the result fma(alpha, sum, label term).  The order depends on C and on the
 * row's length alone; no atomics: two launches are bitwise equal.  offsets and cols are clamped as above.
 * One launch; nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): null F_in, F_out, labels or offsets; F_out == F_in (other rows still read F_in); null
 * cols or vals with nnz > 0; N <= 0, N or nnz >= 2^31, nnz < 0; C < 2 or C > 1024; alpha outside [0, 1] or NaN; a misaligned
 * pointer. */
int32_t cclip_label_spread_groups(int32_t C);
int cclip_label_spread_step(const float* F_in, float* F_out, int64_t N, int32_t C, const int32_t* labels,
                            const float* class_weight, const int64_t* offsets, const int32_t* cols, const float* vals,
                            int64_t nnz, float alpha, float* delta_row, hipStream_t stream);

/* ---- label spreading: the read-out (csrc/label_spread.hip) -----------------------------------------------------------------
 * F fp32 [N, C] contiguous, non-negative.  Per row, z = sum_c F_ic (lane c of CW adds classes c, c + CW, .. ascending, then a
 * fixed tree):
 *   z > 0:   dist[i, :] = p = F / z;  pred[i] = the argmax of F itself, the lowest class among equal values;  conf[i] = max p;
 *            cert[i] = 1 - H(p) / log C,  H = -sum_c p log p  with 0 log 0 = 0
 *   z == 0:  (no labelled row reaches the row) pred = -1, conf = cert = 0, dist row 0: no division, no NaN.  A z below 0
 *            (F is not non-negative) is treated the same.
 *   a NaN in the row: pred = -1, conf, cert and the dist row NaN; no other row is touched.
 * dist fp32 [N, C] may be NULL; pred int32 [N], conf, cert fp32 [N].  One launch, no atomics; nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): null F, pred, conf or cert; N <= 0 or N >= 2^31; C < 2 or C > 1024; a misaligned pointer. */
int cclip_label_spread_finish(const float* F, int64_t N, int32_t C, float* dist, int32_t* pred, float* conf, float* cert,
                              hipStream_t stream);

/* ---- row sampling: temperature, top-k, nucleus and the draw in one launch (csrc/sample_rows.hip, fp32 only) ----
 * One token per row of logits [n, V] (row stride ld >= V elements), for every row r with done[r] == 0:
 *   p        = softmax(row * inv_temperature)
 *   order    : the tokens by (logit descending, id ascending), the fp32 logits compared as they are (-0 == +0)
 *   top-k    : keeps the first top_k tokens of that order (0, or any value >= V: all)
 *   top-p    : among those a token is kept if and only if the mass of the tokens strictly ahead of it is <= top_p (so the
 *              first is always kept; 1 = off)
 *   n_kept   = the size of the kept set, kept_mass = Z = its share of the row's mass
 *   token    : walking the kept tokens in ascending id order, the first whose running kept mass exceeds u[r] * Z
 *              (u[r] in [0, 1); values outside are clamped into [0, 1 - 2^-24])
 *   logprob  = log p[token] (of the full softmax, not the renormalised one)
 *   done[r]  becomes 1 when token == stop_token.
 * A row with done[r] != 0 gets token 0, logprob 0, n_kept 0, kept_mass 0 and done[r] is left alone.  -inf logits are legal
 * (p = 0, never drawn while the row has a finite logit); a row with a NaN, a +inf or no finite logit is undefined (some token in
 * [0, V) comes out, nothing is accessed out of bounds).  token, logprob, n_kept, kept_mass, u and done are [n] contiguous.
 * Masses are 64-bit integers (2^-40 of the row's largest term per unit; a term that is positive in fp32 weighs at least one
 * unit), so every sum is exact and independent of the order it is taken in: no floating-point sum, no floating-point
 * atomic, two launches are bitwise equal and a row's outputs do not depend on n.  One 256-thread work-group per row, six
 * passes over the row, no workspace.  Nothing is read on the host.
 * CCLIP_ERR_ARG (nothing launched): a null pointer; n <= 0; V < 1 or V > 65536; ld < V; top_k < 0; top_p outside (0, 1];
 * inv_temperature not a positive finite number. */
int cclip_sample_rows(const float* logits, int64_t ld, int32_t n, int32_t V, float inv_temperature, int32_t top_k,
                      float top_p, const float* u, int32_t stop_token, int32_t* done, int32_t* token, float* logprob,
                      int32_t* n_kept, float* kept_mass, hipStream_t stream);

/* ---- loss side (fp32) ------------------------------------------------------------------------
 * cclip_l2norm_fwd/bwd: y = x / ||x||_2 per row (image_features / image_features.norm(dim=1)).
 *   No epsilon, as in the reference: a row of zeros gives y = 0 * rsqrt(0) = NaN in every column and inv_norm = +inf - what
 *   x / x.norm() gives in torch; other rows are unaffected.
 * cclip_xent_rows: per row r with label labels[r]: loss_row = logsumexp(row) - row[label]
 *   (0 when label == ignore_index), pred = argmax(row) (first max), and, if dlogits != NULL,
 *   dlogits = (softmax(row) - onehot) * grad_scale (fp32, may alias logits; or bf16, must not);
 *   rowdot (optional) = sum_c dlogits[c] * logits[c]  (the d/d(logit_scale) contribution of the row);
 *   a row is ignored (loss 0, a gradient row of exact zeros, rowdot 0) when label == ignore_index, label < 0 or label >= C.
 *   FINITE LOGITS ONLY: both callers (clip/loss.py, clip_caption/model.py) pass GEMM outputs and nothing masks a logit.  A -inf
 *   that is the first element a lane reads (any of the first 64 columns) turns the row's loss and gradient into NaN (the running
 *   maximum forms exp(-inf - -inf)); a -inf in a later column gets probability 0 and leaves loss, gradient and pred those of
 *   the finite columns, but rowdot (0 * -inf) is NaN; a NaN or +inf logit is undefined.
 *   l2norm_bwd's mul_dev (optional) is a device scalar the result is multiplied by (upstream dloss).
 *   Replaces torch.nn.CrossEntropyLoss + torch.argmax of CLIP/train.py:162-173 and
 *   nnf.cross_entropy(ignore_index=0) of CLIP_prefix_caption/train.py:357. */
int cclip_l2norm_fwd(const float* x, int64_t ldx, int32_t rows, int32_t D, float* y, int64_t ldy,
                     float* inv_norm, hipStream_t stream);
int cclip_l2norm_bwd(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* inv_norm,
                     int32_t rows, int32_t D, float* dx, int64_t lddx, const float* mul_dev,
                     hipStream_t stream);
int cclip_xent_rows(const float* logits, int64_t ld, int32_t R, int32_t C, const int32_t* labels,
                    int32_t ignore_index, float grad_scale, float* loss_row, int32_t* pred,
                    void* dlogits, int32_t dlogits_is_bf16, int64_t ldd, float* rowdot, hipStream_t stream);
/* cclip_xent_rows_classes: the class-aware form (fp32 only).  Row r carries row_class[r], column c carries col_class[c];
 *   the positives of row r are P = { c : col_class[c] == row_class[r] }, empty when row_class[r] < 0 (a negative id means
 *   "unlabelled": such a row contributes nothing, such a column is a negative for every row).  Uniform soft targets over P:
 *   loss_row = logsumexp(row) - mean_{c in P} row[c] (0 when P is empty), pred = argmax(row) (first max),
 *   hit = 1.0f when row_class[r] >= 0 and col_class[pred] == row_class[r], else 0.0f,
 *   dlogits = (softmax(row) - [c in P] / |P|) * grad_scale (fp32, may alias logits; an all-zero row when P is empty),
 *   rowdot = sum_c dlogits[c] * logits[c] (written only together with dlogits).  Every output pointer is optional.
 *   One wave per row, no atomics: two launches are bitwise equal.
 *   CCLIP_ERR_ARG (nothing launched): null logits, row_class or col_class; R <= 0 or C <= 0; ld < C; dlogits with ldd < C. */
int cclip_xent_rows_classes(const float* logits, int64_t ld, int32_t R, int32_t C, const int32_t* row_class,
                            const int32_t* col_class, float grad_scale, float* loss_row, int32_t* pred, float* hit,
                            float* dlogits, int64_t ldd, float* rowdot, hipStream_t stream);
/* cclip_sigmoid_rows: the pairwise sigmoid (SigLIP) row loss (fp32 only), classes as for cclip_xent_rows_classes.  With
 *   b = *bias_dev (a device scalar: nothing is read on the host), u = row[c] + b and y = +1 when row_class[r] >= 0 and
 *   col_class[c] == row_class[r], else -1 (a column with a negative id is a negative for every labelled row):
 *   loss_row = sum_c softplus(-y u), dlogits = -y sigmoid(-y u) * grad_scale (fp32, may alias logits),
 *   rowdot = sum_c dlogits[c] * logits[c] (logits, not u: the d/d(logit_scale) term of the row), rowsum = sum_c dlogits[c]
 *   (the d/d(bias) term of the row); rowdot and rowsum are written only together with dlogits.  A row with row_class[r] < 0
 *   is unlabelled: loss_row, rowdot and rowsum are 0 and its dlogits row is all zeros.  For every row pred = argmax(row)
 *   (first max) and hit = 1.0f when row_class[r] >= 0 and col_class[pred] == row_class[r], else 0.0f.  Every output pointer
 *   is optional.  softplus and sigmoid are formed from exp(-|u|), so |u| = 100 gives finite losses and |dlogits| <=
 *   grad_scale.  One wave per row, one sweep, no atomics: two launches are bitwise equal.
 *   CCLIP_ERR_ARG (nothing launched): null logits, row_class, col_class or bias_dev; R <= 0 or C <= 0; ld < C; dlogits with
 *   ldd < C. */
int cclip_sigmoid_rows(const float* logits, int64_t ld, int32_t R, int32_t C, const int32_t* row_class,
                       const int32_t* col_class, const float* bias_dev, float grad_scale, float* loss_row, int32_t* pred,
                       float* hit, float* dlogits, int64_t ldd, float* rowdot, float* rowsum, hipStream_t stream);
/* cclip_kl_rows: the distillation row loss (fp32 only).  l = row r of logits [R, C] (leading dimension ld), g = row r of
 *   teacher [R, C] (leading dimension ldt, independent of ld; never written), lse = logsumexp:
 *   p_t[c] = exp(g[c] - lse(g)), p_s[c] = exp(l[c] - lse(l)),
 *   loss_row = sum_c p_t[c] * ((g[c] - lse(g)) - (l[c] - lse(l)))   (KL(teacher || student); a cell with p_t == 0 adds 0, so
 *   a teacher cell of -inf contributes exactly nothing), dlogits = (p_s - p_t) * grad_scale (fp32, may alias logits),
 *   rowdot = sum_c dlogits[c] * l[c] (written only together with dlogits), pred = argmax(l) (first max), agree = 1.0f when
 *   argmax(l) == argmax(g), else 0.0f (a row without a maximum agrees with nothing).  Every output pointer is optional.  A
 *   teacher row equal to the logits row gives loss_row and dlogits exactly 0.  A NaN in either row makes that row's loss_row
 *   NaN and touches no other row.  One wave per row, two sweeps (row statistics, then loss and gradient), no atomics: two
 *   launches are bitwise equal.
 *   CCLIP_ERR_ARG (nothing launched): null logits or teacher; R <= 0 or C <= 0; ld < C; ldt < C; dlogits with ldd < C. */
int cclip_kl_rows(const float* logits, int64_t ld, const float* teacher, int64_t ldt, int32_t R, int32_t C, float grad_scale,
                  float* loss_row, int32_t* pred, float* agree, float* dlogits, int64_t ldd, float* rowdot,
                  hipStream_t stream);
/* out (+)= alpha * (mul_dev ? *mul_dev : 1) * sum_i a[i] * (b ? b[i] : 1)   (single block, deterministic) */
int cclip_reduce_dot(const float* a, const float* b, int64_t n, float alpha, const float* mul_dev, float* out,
                     int32_t accumulate, hipStream_t stream);

/* ---- optimiser over the flat parameter arena -------------------------------------------------
 * mode 0: transformers.AdamW (CLIP/train.py:143): p -= lr*sqrt(bc2)/bc1 * m/(sqrt(v)+eps), then
 * p -= lr*wd*p.  mode 1: torch.optim.AdamW.  grad is multiplied by grad_scale first.  If
 * bf16_shadow != NULL the bf16 compute copy of the weights is rewritten in the same pass.
 * n % 4 == 0, buffers 16-byte aligned, step >= 1. */
int cclip_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int32_t step,
                     int32_t correct_bias, float grad_scale, int32_t mode, void* bf16_shadow,
                     hipStream_t stream);
/* cclip_adamw_step with parameter groups, a clip coefficient from a device scalar and an EMA of the new masters, one launch.
 *   groups: chunk_group[c] (uint8, device) names the group of elements [64 c, 64 c + 64) of THIS range (the pointer is already
 *     offset to the range's first chunk; ceil(n / 64) entries are read); lr[] / weight_decay[] are HOST arrays of n_groups
 *     entries, copied into a by-value kernel argument at every call (no device copy, no synchronisation).  A table entry
 *     >= n_groups is the CALLER's to avoid: the kernel does not check it; it can reach no memory outside the argument (the
 *     argument has 256 entries, the table is uint8) and takes lr = weight_decay = 0 - the moments move, the parameter stays.
 *   scalar: with sumsq_dev != NULL the gradient is multiplied by
 *       grad_scale * min(1, max_norm / (|grad_scale| * sqrt(*sumsq_dev) + 1e-6))
 *     instead of grad_scale: torch.nn.utils.clip_grad_norm_'s coefficient for gradients grad_scale * grad whose sum of squares
 *     BEFORE the scaling is *sumsq_dev (cclip_sumsq_f32).  With skip_nonfinite != 0 and *sumsq_dev inf or NaN the launch writes
 *     nothing at all (p, m, v, ema and shadow keep their bits); with skip_nonfinite == 0 the step is applied with whatever
 *     coefficient results (0 for inf, 1 for NaN).
 *   ema != NULL: ema = ema_decay * ema + (1 - ema_decay) * p_new per element (fp32, 16-byte aligned, 0 <= ema_decay <= 1).
 *   The shadow is written as by cclip_adamw_step.  One group, sumsq_dev == NULL and ema == NULL give cclip_adamw_step's bits.
 *   CCLIP_ERR_ARG (nothing launched): what cclip_adamw_step refuses; null chunk_group / lr / weight_decay; n_groups outside
 *   [1, 256]; sumsq_dev with a max_norm that is not finite and > 0; ema misaligned or ema_decay outside [0, 1]. */
int cclip_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const uint8_t* chunk_group, const float* lr, const float* weight_decay, int32_t n_groups,
                            float beta1, float beta2, float eps, int32_t step, int32_t correct_bias, float grad_scale,
                            int32_t mode, void* bf16_shadow, const float* sumsq_dev, float max_norm, int32_t skip_nonfinite,
                            float* ema, float ema_decay, hipStream_t stream);
/* blocks of the cclip_adamw_step / cclip_adamw_step_groups launch over n elements (256 threads, two float4 groups a grid
 * stride apart per trip: a thread takes a second trip when n / 4 > 2 * 256 * blocks); 0 for an n the calls refuse */
int32_t cclip_adamw_grid(int64_t n);
/* out (+)= sum_i x[i]^2 over n fp32 elements (n % 4 == 0, x 16-byte aligned), fp32 only, two launches, no float atomics:
 * stage 1 runs B = cclip_sumsq_workspace(n) / 4 = min(ceil(n / 1024), 1024) blocks of 256 threads; thread t of block b folds
 * the float4 groups b * 256 + t, + 256 B, ... element by element into one fma chain, the block adds its chains by a 6-level
 * butterfly and its 4 wave sums in order, and writes partials[b]; stage 2 (one block) starts from *out when accumulate != 0,
 * else from 0, and adds partials[0 .. B) in ascending order.  Two calls on the same data give equal bits.  A NaN or an inf in
 * x (or a square that overflows) makes *out non-finite; when *out is non-finite after the fold and nonfinite_count != NULL,
 * one thread adds 1 to that int32 with a plain load and store.  partials: at least cclip_sumsq_workspace(n) bytes of device
 * memory (0 for an n the call refuses), 4-byte aligned, contents undefined afterwards.
 * CCLIP_ERR_ARG (nothing launched): null x, partials or out; n <= 0 or n % 4 != 0; x not 16-byte aligned. */
int cclip_sumsq_f32(const float* x, int64_t n, float* partials, float* out, int32_t accumulate, int32_t* nonfinite_count,
                    hipStream_t stream);
int64_t cclip_sumsq_workspace(int64_t n);
int cclip_cast_f32_to_bf16(const float* in, void* out, int64_t n, hipStream_t stream);
/* Batched out-of-place transpose of 16-bit matrices (bf16 or fp16: elements are moved, not interpreted): for i < n_matrices,
 * dst_base[table[i].dst_off ...] as [cols, rows] = transpose of src_base[table[i].src_off ...] as [rows, cols];
 * table_dev = n_matrices x {src_off, dst_off, rows, cols} int64 in DEVICE memory (element offsets), max_tiles = the largest
 * ceil(rows/64) * ceil(cols/64) of the batch.  Rebuilds the transposed weight shadows the dgrad GEMMs read (one launch per
 * optimiser step), so that dX = dY . W runs in the forward operand layout. */
int cclip_transpose16_batched(const void* src_base, void* dst_base, const int64_t* table_dev, int32_t n_matrices,
                              int32_t max_tiles, hipStream_t stream);
/* x[i] *= alpha over n fp32 elements (n % 4 == 0, 16-byte aligned).  The fp16 operand mode runs its backward under a static
 * power-of-two loss scale (the 16-bit gradient stream of a mean loss over thousands of rows would otherwise sink into
 * fp16 subnormals); this undoes it on the flat gradient arena. */
int cclip_scale_f32(float* x, int64_t n, float alpha, hipStream_t stream);

/* ---- device-side preprocess --------------------------------------------------------------------
 * openai/CLIP's _transform(n) = Resize(n, BICUBIC) -> CenterCrop(n) -> ToTensor -> Normalize on a decoded 8-bit RGB image
 * (HWC, 3 bytes per pixel), bit-identical to the PIL + numpy pipeline the reference runs in DataLoader workers
 * (CLIP/train.py:56).  Two launches per image: a horizontal 8-bit resampling pass (PIL's integer resampler: windows and
 * 2^22-scaled integer coefficients per output sample, computed on the host) over the rows the vertical pass needs and the
 * columns that survive the crop, then the vertical pass fused with crop + (u8/255 - mean)/std -> fp32 [3, n, n].
 * mean3 / std3 are HOST pointers to 3 floats. */
int cclip_resample_h_u8(const uint8_t* in, int64_t in_ld, int32_t rows, const int32_t* bounds, const int32_t* kk,
                        int32_t ksize, int32_t out_w, uint8_t* out, int64_t out_ld, hipStream_t stream);
int cclip_resample_v_norm(const uint8_t* tmp, int64_t tmp_ld, int32_t row0, const int32_t* bounds, const int32_t* kk,
                          int32_t ksize, int32_t n, const float* mean3, const float* std3, float* out, hipStream_t stream);

/* Region preprocess: K boxes of decoded photos -> out fp32 [K, 3, n, n], every box bit-identical to _transform(n) of the
 * cropped box, in three launches whatever K is; the windows and coefficients are computed on the device.
 * One descriptor per box, filled on the host (clip/preprocess_device.py:roi_descriptors) and passed twice: `desc_host` is a
 * HOST copy that the launcher checks before it launches anything (it is not kept), `desc` the same records in device memory.
 * The kernels read `desc` only, and a launcher cannot compare the two without a read-back: the bounds guarantee below holds
 * only if the caller passes two identical copies (clip.DevicePreprocess uploads `desc` from `desc_host` and edits neither).
 *   src_off, src_ld  byte offset of the box's top-left pixel in `src` and the row stride in bytes of its photo (HWC uint8
 *                    RGB; several photos of different sizes may be packed into one buffer);
 *   tmp_off          byte offset of the box's rows in the 8-bit intermediate (rows * n * 3 bytes, box after box);
 *   w, h             box size; nw, nh: its size after Resize(n) on the shorter side; left, top: the centre crop;
 *   row0, rows       the input rows (relative to the box) that the n surviving output rows read.
 * Tables: bounds int32 [K, 2, n, 2] = (first index, count), kk int32 [K, 2, n, ksize_max]; axis 0 horizontal, 1 vertical;
 * indices are relative to the box; only the first `count` coefficients of a row are written.  ksize_max: at least the largest
 * ksize = 2 * ceil(2 * max(in / out, 1)) + 1 of any box and axis, at most 257 (a downscale factor of 64).
 * CCLIP_ERR_ARG (nothing launched): a null pointer; K, n, ksize_max, src_bytes or tmp_bytes <= 0; ksize_max above 257 or
 * below what a box needs; a descriptor whose nw / nh / left / top / row0 / rows do not fit n and its w, h, or whose source or
 * intermediate extent leaves [0, src_bytes) / [0, tmp_bytes); src_ld above 2^36.  mean3 / std3 are HOST pointers to 3 floats. */
typedef struct cclip_roi_desc {
  int64_t src_off, src_ld, tmp_off;
  int64_t w, h, nw, nh, left, top, row0, rows;
} cclip_roi_desc;
int cclip_roi_coeffs(const cclip_roi_desc* desc_host, const cclip_roi_desc* desc, int32_t K, int32_t n, int32_t ksize_max,
                     int32_t* bounds_out, int32_t* kk_out, hipStream_t stream);
int cclip_roi_resample_h(const uint8_t* src, int64_t src_bytes, const cclip_roi_desc* desc_host, const cclip_roi_desc* desc,
                         int32_t K, int32_t n, int32_t ksize_max, const int32_t* bounds, const int32_t* kk, uint8_t* tmp,
                         int64_t tmp_bytes, hipStream_t stream);
int cclip_roi_resample_v_norm(const uint8_t* tmp, int64_t tmp_bytes, const cclip_roi_desc* desc_host, const cclip_roi_desc* desc,
                              int32_t K, int32_t n, int32_t ksize_max, const int32_t* bounds, const int32_t* kk,
                              const float* mean3, const float* std3, float* out, hipStream_t stream);

/* ---- fp8 (OCP e4m3) inference projections --------------------------------------------------------
 * BASELINE.json configs[4] (ViT-L/14@336px encode_image, fp8 MFMA path).  No reference behaviour exists for fp8
 * (the reference runs fp16 / fp32): parity of this path is unpinned and bounded against the fp32 oracle by test.
 * cclip_quantize_rows_fp8: x16 [rows, cols] (cols % 8 == 0) -> e4m3 bytes [rows, cols] and scale[r] = amax_r / 448
 *   (1 for an all-zero row), x ~= scale[r] * fp8.  Per token for activations, per output channel for weights.
 * cclip_gemm_fp8: out16[m][n] = act(scale_a[m] * scale_b[n] * sum_k A8[m][k] * B8[n][k] + bias[n]); A8 [M,K], B8 [N,K]
 *   K-contiguous e4m3, K % 16 == 0, leading dimensions % 16 == 0, 16-byte aligned; act NONE or QUICKGELU.
 *   v_mfma_scale_f32_16x16x128_f8f6f4 (the form that runs at 2x the bf16 rate on gfx950), block scales fixed at 1. */
int cclip_quantize_rows_fp8(const void* x_bf16, int64_t ldx, int32_t rows, int32_t cols, void* out_fp8, int64_t ldo,
                            float* scale, hipStream_t stream);
/* LayerNorm (as cclip_layernorm_fwd) whose output is written as e4m3 rows + per-row scale: the A operand of the LN-fed
 * projections (qkv, fc) with no separate quantisation pass. */
int cclip_layernorm_fwd_fp8(const float* x, int64_t ldx, int32_t rows, int32_t D, const float* gamma, const float* beta,
                            float eps, void* out_fp8, int64_t ldo, float* scale, hipStream_t stream);
int cclip_gemm_fp8(const void* A8, int64_t lda, const float* scale_a, const void* B8, int64_t ldb, const float* scale_b,
                   int32_t M, int32_t N, int32_t K, const float* bias, int32_t act, void* out_bf16, int64_t ldc,
                   hipStream_t stream);
/* Round 2: block-scaled (MX) A operands, so that the projections whose input no single workgroup sees a whole row of
 * (out-proj <- attention, c_proj <- the fc GEMM's epilogue) can run in e4m3 too.
 * cclip_quantize_mx_fp8: x16 [rows, cols] (cols % 32 == 0) -> e4m3 [rows, cols] + one E8M0 byte per (row, 32 columns):
 *   x ~= 2^(e - 127) * fp8 with e the smallest exponent that keeps the block's amax within +-448.
 *   Block-scale layout (both functions): K-tile major [cols/128][rows][4] bytes - the scale of (row r, block b) is byte
 *   (b >> 2) * ld + 4 r + (b & 3), ld >= 4 * rows = the byte distance between the planes of consecutive 128-column groups.
 * cclip_gemm_fp8_ex: cclip_gemm_fp8 in descriptor form with
 *   - block_scale_a != NULL: A carries E8M0 block scales (K % 128 == 0, layout above) applied by the MFMA itself
 *     (v_mfma_scale_f32_16x16x128_f8f6f4 takes one scale byte per lane = per (row, 32-deep k block)); scale_a is not read;
 *   - exactly one output: out16 (16-bit), out_fp8 + out_block_scale (e4m3 + E8M0 per 32 output columns, N % 64 == 0: the
 *     block-scaled A operand of the NEXT GEMM written straight from the epilogue), or out_f32 = residual + result (fp32
 *     residual stream, shared leading dimension ldf; may alias).
 *   Kernel set: act NONE with any combination above except (block scales, fp8 out); act QUICKGELU with row-scaled A and
 *   out16 or out_fp8; anything else returns status 1. */
int cclip_quantize_mx_fp8(const void* x_bf16, int64_t ldx, int32_t rows, int32_t cols, void* out_fp8, int64_t ldo,
                          void* block_scale, int64_t ld_block_scale, hipStream_t stream);
typedef struct cclip_fp8_gemm_desc {
  const void* A; int64_t lda; const float* scale_a;
  const void* block_scale_a; int64_t ld_block_scale_a;
  const void* B; int64_t ldb; const float* scale_b;
  int32_t M, N, K;
  const float* bias;
  int32_t act;
  void* out16; int64_t ldc;
  void* out_fp8; int64_t ld_out_fp8; void* out_block_scale; int64_t ld_out_block_scale;
  float* out_f32; const float* residual; int64_t ldf;
} cclip_fp8_gemm_desc;
int cclip_gemm_fp8_ex(const cclip_fp8_gemm_desc* d, hipStream_t stream);

/* ---- native driver of one KV-cached GPT-2 decode step ------------------------------------------
 * One call = the whole per-token launch sequence (per layer: ln_1, qkv GEMM, cache append, decode attention,
 * out-proj GEMM + residual, ln_2, fc GEMM + activation, proj GEMM + residual; then optionally ln_f + tied lm_head)
 * for n_seq sequences - the body of the reference's generate_beam / generate2 loops
 * (CLIP_prefix_caption/test.py:381,468), which re-run `model.gpt(inputs_embeds=generated)` on the whole sequence.
 * Issued from C++ so that a step costs ~100 kernel launches, not ~100 Python -> ctypes round trips.
 * x: fp32 [n_seq, width], in = token embedding + position embedding of position `pos`, out = final hidden state.
 * kcache / vcache: 16-bit, element (layer l, sequence b, position s, column c) at l*ld_layer + b*ld_seq + s*width + c;
 * positions [0, pos) must be filled; position pos is written.  scratch16: n_seq * (5*width + hidden) 16-bit elements.
 * linear_layout: 1 = nn.Linear [out,in] weights, 0 = GPT-2 Conv1D [in,out].  logits == NULL skips the head. */
typedef struct cclip_block_ptrs {
  const float* ln1_w; const float* ln1_b; const void* w_qkv; const float* b_qkv; const void* w_o; const float* b_o;
  const float* ln2_w; const float* ln2_b; const void* w_fc; const float* b_fc; const void* w_proj; const float* b_proj;
} cclip_block_ptrs;
typedef struct cclip_decode_desc {
  int32_t n_layer, n_seq, width, heads, hidden, act, linear_layout, pos;
  const cclip_block_ptrs* blocks;
  float* x;
  void* kcache; void* vcache;
  int64_t ld_layer, ld_seq;
  void* scratch16;
  const float* lnf_w; const float* lnf_b; const void* wte16; int32_t vocab; float* logits; int64_t ld_logits;
} cclip_decode_desc;
int cclip_gpt2_decode_step(const cclip_decode_desc* d, hipStream_t stream);

/* ---- persistent KV-cached beam search -------------------------------------------------------------
 * Replaces the body of the reference's generate_beam loop (CLIP_prefix_caption/test.py:380-434, application.py:176-222:
 * `model.gpt(inputs_embeds=generated)` on the growing sequence, temperature, softmax(-1).log(), the stopped-beam rule,
 * length-normalised top-k over [beams x vocab], token append, beam reorder, next-token embedding) with ONE kernel launch for
 * `n_steps` decode steps: one workgroup per CU, phases separated by a grid barrier (csrc/decode_persist.hip).
 * step: as for cclip_gpt2_decode_step (Conv1D weight layout only, n_seq = beam count <= 8, n_layer <= 24, head_dim 64);
 *   step.pos = position of the first token to be decoded (= length of the prefilled prefix); step.x is written by the
 *   selection (token embedding + position embedding of the chosen tokens) and need not be initialised when first = 1;
 *   step.logits (optional, fp32 [n_seq, ld_logits]) receives each step's logits.
 * first = 1: `first_logits` [vocab] are the prefill's last-position logits and the first selection is the one-sequence form
 *   (test.py:396-405: top-k of one row, scores = its log-probabilities); the key / value rows of the prefix must be in cache
 *   slot 0 and `slot_of` zero.  first = 0 continues a search from the state the previous call left.
 * slot_of: int32 [max_len][8]: cache slot holding beam b's key / value of position t (beam reorder permutes this table; the
 *   cache itself is never copied).  tokens: int32 [n_seq][ld_tokens], state[4] columns valid on entry (prompt tokens of row 0
 *   when first = 1) - one more per selection.  scores / seq_lengths / is_stopped: [n_seq] (written when first = 1).
 * state: int32 [8]: [0] barrier counter and [1] error flag (cleared by every call; error = a grid barrier timed out),
 *   [2] set once every beam has stopped, [3] number of selections made by then (the reference's loop breaks there),
 *   [4] token columns.  Zero [2..4] (or set [4] to the prompt length) before the first call.
 * select_ws: fp32 [256 * 8 * 20].  grid_cap: 0, or a cap on the number of workgroups (tests).
 * After every beam has stopped the remaining steps are skipped (the kernel exits); results are those of the loop's break. */
typedef struct cclip_beam_desc {
  cclip_decode_desc step;
  int32_t n_steps, first, stop_token, ld_tokens, max_len, grid_cap;
  float temperature;
  const float* first_logits;
  const float* wte_f32; const float* wpe_f32;
  int32_t* slot_of; int32_t* tokens;
  float* scores; float* seq_lengths; int32_t* is_stopped;
  int32_t* state; float* select_ws;
} cclip_beam_desc;
int cclip_gpt2_beam_search(const cclip_beam_desc* d, hipStream_t stream);

/* ---- batched persistent beam search --------------------------------------------------------------
 * cclip_gpt2_beam_search for n_cap captions at once (csrc/decode_persist_batch.hip): n_cap x beams rows (<= 64, beams <= 8)
 * share every weight read and every phase hand-over of a step.  Geometry limits as cclip_gpt2_beam_search.  Always starts
 * with the one-row selection of every caption from first_logits ([n_cap][vocab] fp32) and runs up to n_steps decode steps.
 * step.n_seq = n_cap * beams; row r = c * beams + b is beam b of caption c, and caption c owns cache slots (kcache /
 * vcache dimension 1) c*beams .. c*beams+beams-1 with its prefix (positions [0, step.pos)) in slot c*beams.
 * max_len: cache positions per slot (step.ld_seq >= max_len * width), > step.pos; wpe_f32 must hold max_len rows.
 * slot_of: int32 [n_cap][max_len][8], zero before the call.  tokens: int32 [n_cap*beams][ld_tokens], ld_tokens > n_steps.
 * scores / seq_lengths / is_stopped: [n_cap*beams].  state: int32 [8] ([0] counter, [1] error = a hand-over timed out,
 * [2] captions stopped); cap_state: int32 [n_cap][8] ([2] stopped, [3] selections made by then); both are cleared by every
 * call.  select_ws: fp32 [n_cap * 256 * 8 * 20].  A caption's results do not depend on the other captions of the launch. */
typedef struct cclip_beam_batch_desc {
  cclip_decode_desc step;
  int32_t n_cap, beams, n_steps, stop_token, ld_tokens, max_len, grid_cap;
  float temperature;
  const float* first_logits;
  const float* wte_f32; const float* wpe_f32;
  int32_t* slot_of; int32_t* tokens;
  float* scores; float* seq_lengths; int32_t* is_stopped;
  int32_t* state; int32_t* cap_state; float* select_ws;
} cclip_beam_batch_desc;
int cclip_gpt2_beam_search_batch(const cclip_beam_batch_desc* d, hipStream_t stream);

/* ---- relevance overlays --------------------------------------------------------------------------
 * N patch-relevance vectors and their images -> N finished 8-bit RGB overlays in one launch (csrc/relevance_overlay.hip; the
 * reference's show_image_relevance, attention.py:77-96).  For output pixel (y, x) of overlay n, everything in fp32:
 *   bil(src, L, i): F.interpolate(mode="bilinear", align_corners=False) - s = max((i + 0.5) L / S - 0.5, 0), i0 = floor(s),
 *                   i1 = min(i0 + 1, L - 1), weight s - i0, separable in y and x;
 *   u = bil of the g x g grid, m = (u - min u) / (max u - min u) over the S x S pixels (0 when the range is 0);
 *   v_c = bil of image channel c, xn_c = (v_c - min v) / (max v - min v) over all 3 S S values (0 when the range is 0);
 *   k = min(floor(255 m), 255), cam_c = lut[k][c] + xn_c, M = max cam over all 3 S S values;
 *   out[n][y][x][c] = floor(255 (cam_c / M)), 0 when M == 0 (values outside [0, 255] - a negative table entry - saturate).
 * rel: fp32 [N][g*g].  images: fp32 [3][R][R] per overlay, overlay n's at images + n * image_stride floats; image_stride 0 =
 *   one image shared by all N maps, otherwise >= 3 R R.  lut: fp32 [256][3].  out: uint8 [N][S][S][3], any alignment.
 * map_out: NULL, or fp32 [N][S][S] that receives m.  1 <= g, R, S <= CCLIP_OVERLAY_MAX_SIDE.
 * One work-group per overlay, no atomics: two calls give the same bytes. */
#define CCLIP_OVERLAY_MAX_SIDE 16384
int cclip_relevance_overlay(const float* rel, int32_t N, int32_t g, const float* images, int64_t image_stride, int32_t R,
                            const float* lut, int32_t S, uint8_t* out, float* map_out, hipStream_t stream);

/* ---- dense zero-shot maps ------------------------------------------------------------------------
 * Per-patch class probabilities and the label map / picture made from them (csrc/dense_classes.hip); all fp32, no fp16 twin.
 * How a pixel's label is chosen, stored and painted is csrc/label_pixels.h, one writer for this kernel and cclip_dense_stitch.
 *
 * cclip_dense_class_probs: feat [M][E] with row stride ldf (floats), M = B * P patch rows, image b owns rows b P .. b P + P - 1;
 *   text [C][E] contiguous.  Neither side needs unit rows:
 *     cos[m][c] = <feat_m, text_c> / (|feat_m| |text_c|), taken as 0 when either norm is 0 (no epsilon is added to a norm, as
 *                 in cclip_l2norm_fwd; a zero feature row therefore gets the uniform distribution instead of NaN)
 *     probs[b][c][p] = softmax over c of scale * cos[b P + p][c]        class-major [B][C][P]: probs[b][c] is one g x g map
 *   logits_out: NULL, or [B][C][P] that receives scale * cos.  One wave per row, the text staged through LDS in tiles, fp32
 *   accumulation in a fixed order, no atomics: two calls give equal bytes.
 *   CCLIP_ERR_ARG: a null pointer; M < 1, P < 1 or M not a multiple of P; C outside [1, 255]; E outside [4, 1024] or not a
 *   multiple of 4; ldf < E or not a multiple of 4; feat or text not 16-byte aligned.
 *
 * cclip_dense_label_map: probs [B][C][g][g]; every class map is upsampled to S x S with cclip_relevance_overlay's bil()
 *   (F.interpolate(mode="bilinear", align_corners=False)), its source coordinate ((2 i + 1) g - S) / (2 S) formed in integers
 *   so that the weights are one rounding from exact, and per output pixel
 *     conf   [B][S][S] fp32  = the largest upsampled probability
 *     labels [B][S][S] uint8 = the LOWEST class index that reaches it, 255 when conf < min_conf
 *   overlay (NULL, or uint8 [B][S][S][3]; needs palette uint8 [256][3], row 255 = the colour of "no class"):
 *     palette[label][ch] without a photo; with photo (uint8 [B][S][S][3], already S x S)
 *     (photo * (256 - a8) + palette[label][ch] * a8 + 128) >> 8, a8 an integer in [0, 256] - exact given the labels.
 *   labels, overlay and photo may have any alignment; C in [1, 255]; 1 <= g, S <= CCLIP_OVERLAY_MAX_SIDE.  No atomics: two
 *   calls give equal bytes. */
int cclip_dense_class_probs(const float* feat, int64_t ldf, int64_t M, int32_t P, const float* text, int32_t C, int32_t E,
                            float scale, float* probs, float* logits_out, hipStream_t stream);
int cclip_dense_label_map(const float* probs, int32_t B, int32_t C, int32_t g, int32_t S, float min_conf, uint8_t* labels,
                          float* conf, const uint8_t* palette, const uint8_t* photo, int32_t a8, uint8_t* overlay,
                          hipStream_t stream);

/* cclip_dense_stitch (csrc/dense_stitch.hip): K class-map sets probs [K][C][g][g], set k the dense head's answer for the window
 *   boxes[k] = (x0, y0, x1, y1) (int32 [K][4], on the device) of one H x W picture, stitched into the picture's label map,
 *   confidence map and picture in one launch.  Sliding windows, a multi-scale list of squares, or one rectangle over a
 *   non-square picture are all lists of boxes.
 *   Coverage: window k covers pixel (x, y) when x0 <= x < x1, y0 <= y < y1, 1 <= x1 - x0 <= CCLIP_OVERLAY_MAX_SIDE and
 *     1 <= y1 - y0 <= CCLIP_OVERLAY_MAX_SIDE, the sides formed without 32-bit overflow.  An empty, inverted or oversized box
 *     covers nothing; a box may hang over the picture's edge.  The launcher cannot see the boxes: the kernel itself reads
 *     nothing outside probs and boxes for ANY box values.
 *   Sample: s_kc = bil of probs[k][c] at the window-local position (y - y0, x - x0), align_corners=False, the y axis with
 *     scale g / (y1 - y0) and the x axis with g / (x1 - x0), coordinates formed in integers as in cclip_dense_label_map.
 *   Average: over the n covering windows k1 < k2 < .. in ascending k, u_c = ((s_k1c + s_k2c) + ..) / (float)n - the sum seeded
 *     with the first sample, fp32 adds left to right, one division also when n = 1.
 *     conf   [H][W] fp32  = max_c u_c;   0 when n = 0
 *     labels [H][W] uint8 = the LOWEST class reaching conf, 255 when conf < min_conf or n = 0
 *     cover  NULL, or [H][W] uint8 = min(n, 255)
 *     overlay NULL, or uint8 [H][W][3]: the integer formula stated for cclip_dense_label_map on the label (palette [256][3],
 *     photo NULL or uint8 [H][W][3], a8 in [0, 256]) - the same code, csrc/label_pixels.h.
 *   For K = 1, H = W = S and the box (0, 0, S, S), labels, conf and overlay equal cclip_dense_label_map's bit for bit.  There is
 *   no cap on how many windows cover a pixel.  One launch, no atomics, nothing depends on the launch geometry: two calls give
 *   equal bytes.
 *   CCLIP_ERR_ARG, nothing launched: probs, boxes, labels or conf NULL; K outside [1, 65535]; C outside [1, 255]; g, H or W
 *   outside [1, CCLIP_OVERLAY_MAX_SIDE]; overlay without palette, photo without overlay, a8 outside [0, 256]; probs, conf or
 *   boxes not 4-byte aligned.  labels, cover, overlay and photo may have any alignment. */
int cclip_dense_stitch(const float* probs, int32_t K, int32_t C, int32_t g, const int32_t* boxes, int32_t H, int32_t W,
                       float min_conf, uint8_t* labels, float* conf, uint8_t* cover, const uint8_t* palette, const uint8_t* photo,
                       int32_t a8, uint8_t* overlay, hipStream_t stream);

/* Image-guided refinement of dense class maps (prepare and step: csrc/dense_refine.hip; cclip_dense_stitch_maps: csrc/dense_stitch.hip,
 * on the functions cclip_dense_stitch runs; cclip_dense_maps_label: csrc/dense_classes.hip): pixel-adaptive mask refinement (PAMR;
 * Araslanov & Roth, CVPR 2020), stated here from the paper's formulas - this text is the contract, no other implementation was compared.
 *
 * cclip_dense_stitch_maps: cclip_dense_stitch's inputs (probs [K][C][g][g], device boxes int32 [K][4], H, W) and its coverage,
 *   sampling and averaging rules, but the averaged maps themselves are written: maps [C][H][W] fp32 = u_c, 0 where no window
 *   covers the pixel; cover NULL, or uint8 [H][W] = min(n, 255).  max_c maps[c] equals cclip_dense_stitch's conf bit for bit.
 *   CCLIP_ERR_ARG, nothing launched: probs, boxes or maps NULL; K outside [1, 65535]; C outside [1, 255]; g, H or W outside
 *   [1, CCLIP_OVERLAY_MAX_SIDE]; C H W > 2^31 - 1; probs, boxes or maps not 4-byte aligned.  cover may have any alignment.
 *
 * cclip_dense_maps_label: maps [B][C][H][W] fp32 -> conf [B][H][W] = max_c maps, labels = the LOWEST class reaching it, 255 when
 *   conf < min_conf; cover NULL, or uint8 [B][H][W] (an INPUT): where it is 0 the pixel gets label 255 and conf 0 whatever the
 *   maps hold.  overlay, palette, photo, a8 as for cclip_dense_label_map, pictures [B][H][W][3] (the same code,
 *   csrc/label_pixels.h).  cclip_dense_stitch_maps followed by this call with its cover equals cclip_dense_stitch byte for byte.
 *   CCLIP_ERR_ARG, nothing launched: maps, labels or conf NULL; B < 1; C outside [1, 255]; H or W outside
 *   [1, CCLIP_OVERLAY_MAX_SIDE]; B C H W > 2^31 - 1; maps or conf not 4-byte aligned; overlay without palette, photo without
 *   overlay, a8 outside [0, 256].  labels, cover, overlay and photo may have any alignment.
 *
 * The refinement.  guide uint8 [B][H][W][3] (the photo at the maps' size, any alignment), channel value x_k = byte / 255;
 *   dilations d_0 .. d_{D-1} (D ints on the HOST, read during the call), 1 <= D <= CCLIP_REFINE_MAX_DILATIONS,
 *   1 <= d <= CCLIP_REFINE_MAX_DILATION.  Pixel p = (y, x) has N = 8 D neighbours, n = 8 j + e at q_n = clamp(p + d_j o_e) with
 *   o_e = (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1) as (dy, dx), coordinates clamped to the image (replicate
 *   padding); the centre is no neighbour and nothing crosses from one image of the batch to another.
 *     sigma_k(p) = the unbiased standard deviation (divisor 9 D - 1) of x_k over the 9 D taps: the N neighbours and the centre
 *                  once per dilation; formed from integer sums of the bytes, n sum(b^2) - sum(b)^2 exactly
 *     a_n(p)     = -(1/3) sum_k |x_k(p) - x_k(q_n)| / (1e-8 + 0.1 sigma_k(p))
 *     w_n(p)     = softmax over n of a_n(p)
 *     m'_c(p)    = sum_n w_n(p) m_c(q_n)        ascending n, fp32, seeded with the first product, then one fma per neighbour
 *   cclip_dense_refine_prepare writes key [B][H][W][4] fp32: key[0..2] = 1 / (1e-8 + 0.1 sigma_k), key[3] = L(p) =
 *     max_n a_n + log sum_n exp(a_n - max), so that w_n = exp(a_n - L) with no reduction per iteration (expf / logf).
 *   cclip_dense_refine_step runs ONE iteration maps_in -> maps_out, both [B][C][H][W] fp32, with the guide, the key and the
 *     dilations the key was made with; the caller alternates two buffers.  A flat guide gives w_n = 1 / N whatever its colour.
 *   No atomics, nothing depends on the launch geometry: two calls give equal bytes.
 *   CCLIP_ERR_ARG, nothing launched: a NULL pointer; B < 1; H or W outside [1, CCLIP_OVERLAY_MAX_SIDE]; D or a dilation outside
 *   its range; key not 16-byte aligned; prepare: B H W > 2^31 - 1; step: C outside [1, 255], B C H W > 2^31 - 1, maps_in or
 *   maps_out not 4-byte aligned, maps_in and maps_out the same or overlapping buffers. */
#define CCLIP_REFINE_MAX_DILATIONS 6
#define CCLIP_REFINE_MAX_DILATION 24
int cclip_dense_stitch_maps(const float* probs, int32_t K, int32_t C, int32_t g, const int32_t* boxes, int32_t H, int32_t W,
                            float* maps, uint8_t* cover, hipStream_t stream);
int cclip_dense_maps_label(const float* maps, int32_t B, int32_t C, int32_t H, int32_t W, const uint8_t* cover, float min_conf,
                           uint8_t* labels, float* conf, const uint8_t* palette, const uint8_t* photo, int32_t a8,
                           uint8_t* overlay, hipStream_t stream);
int cclip_dense_refine_prepare(const uint8_t* guide, int32_t B, int32_t H, int32_t W, const int32_t* dilations, int32_t D,
                               float* key, hipStream_t stream);
int cclip_dense_refine_step(const float* maps_in, float* maps_out, const uint8_t* guide, const float* key, int32_t B, int32_t C,
                            int32_t H, int32_t W, const int32_t* dilations, int32_t D, hipStream_t stream);

/* cclip_label_components (csrc/label_components.hip): the connected components of labels uint8 [B][H][W], 255 = "none".
 *   Two pixels are joined when they lie in the same image, carry the same label other than 255 and are 4-neighbours
 *   (connectivity 4) or 8-neighbours (connectivity 8); components are the classes of the transitive closure.  Nothing joins
 *   across the images of the batch, nothing wraps from the end of a row to the start of the next.  With the flat index
 *   p = (b H + y) W + x:
 *     root  [B][H][W] int32 = the flat index of the component's FIRST pixel in row-major order, -1 where the label is 255
 *     ids   [B][H][W] int32 = the component's number: 0 .. n - 1 in ascending order of root, -1 for "none"
 *     count [1]       int32 = n, on the device
 *   workspace: int32 [workspace_ints], workspace_ints >= ceil(B H W / CCLIP_COMPONENTS_GROUP) (the per-group root counts);
 *   `ids` holds the union-find parents until the numbering overwrites it.  root, ids, count and workspace must not overlap.
 *   Label equivalence with integer atomicMin, the smaller index always wins: root and ids are canonical forms that do not
 *   depend on the order in which atomics land, so two calls give equal bytes.  Six launches; no kernel waits for another
 *   work-group, every loop moves to strictly smaller indices.
 *   CCLIP_ERR_ARG, nothing launched: a NULL pointer; B < 1; H or W outside [1, CCLIP_OVERLAY_MAX_SIDE]; B H W > 2^31 - 1 (formed
 *   in 64 bits); connectivity other than 4 or 8; root, ids, count or workspace not 4-byte aligned; workspace_ints too small.
 *   labels may have any alignment.
 *
 * cclip_component_stats: what each of the n components is, from the labelling above (the caller reads count first; n sizes the
 *   outputs).  For component i < n:
 *     label[i] uint8, image[i] int32 (the batch index), first[i] int32 (its root index), area[i] int32 (pixels),
 *     box[i] int32 x 4 = (x0, y0, x1, y1), half-open, in the image's own coordinates,
 *     qsum[i] uint64 = the sum over the component's pixels of q(conf), conf fp32 [B][H][W]:
 *       q(v) = (v >= 0) ? min(65536, (uint32)(v * 65536.0f + 0.5f)) : 0, NaN gives 0 (fp32 operations, each rounded once);
 *       the mean confidence is qsum / (65536 area).  conf and qsum are given together or both NULL.
 *   Integer sums, minima and maxima by 32- and 64-bit integer atomics, after the pixels of a wave that share a component have
 *   been combined: two calls give equal bytes.  Pixels whose id lies outside [0, n) are passed over.  n == 0 returns CCLIP_OK
 *   with nothing launched and the outputs neither checked nor touched.
 *   CCLIP_ERR_ARG, nothing launched: labels, root or ids NULL; with n > 0 a NULL label, image, first, area or box; conf without
 *   qsum or qsum without conf; the shape limits above; n < 0 or n > B H W; an int32 / fp32 pointer not 4-byte aligned, qsum
 *   not 8-byte aligned.  labels and label may have any alignment. */
#define CCLIP_COMPONENTS_GROUP 1024
int cclip_label_components(const uint8_t* labels, int32_t B, int32_t H, int32_t W, int32_t connectivity, int32_t* root,
                           int32_t* ids, int32_t* count, int32_t* workspace, int64_t workspace_ints, hipStream_t stream);
int cclip_component_stats(const uint8_t* labels, const float* conf, const int32_t* root, const int32_t* ids, int32_t B, int32_t H,
                          int32_t W, int32_t n, uint8_t* label, int32_t* image, int32_t* first, int32_t* area, int32_t* box,
                          uint64_t* qsum, hipStream_t stream);

/* cclip_label_agreement (csrc/label_agreement.hip): how well pred agrees with gt, both uint8 [B][H][W], as the integer counts
 *   behind mean IoU and boundary IoU (Cheng et al., CVPR 2021; stated from the paper, no bit-level agreement with another
 *   implementation is claimed).  C classes, R = per_image ? B : 1 rows of results (row b of image b, or one row for the batch).
 *     confusion [R][C][C+1] int64: confusion[r][g][p] = pixels with gt == g < C and pred == p < C; column C counts pred == 255
 *                                  ("none").  Pixels with gt == 255 are ignored everywhere.
 *     bad       [R][2]      int64: pixels with gt in [C, 254]; pixels with gt < C and pred in [C, 254].  Such pixels enter no
 *                                  other count.
 *     bands     [R][C][3]   int64: (|G_c|, |P_c|, |G_c n P_c|) for the band half-width d = band; required when d > 0, NULL when
 *                                  d == 0.
 *   Band: pixel p is in the band of a map m when some q with |q_x - p_x| <= d and |q_y - p_y| <= d lies outside the image or
 *   has m[q] != m[p], compared as raw bytes (255 and out-of-range values are values like any other).  Nothing crosses between
 *   the images of a batch, nothing wraps from the end of a row to the start of the next.  G_c = pixels with gt == c in gt's
 *   band; P_c = pixels with pred == c and gt < C in pred's band; ignored and bad pixels are in neither.
 *   accumulate == 0 sets the outputs, accumulate == 1 adds the counts to what they hold (a device-side sum over a dataset).
 *   Integer sums by 32-bit LDS and 64-bit global atomics: two calls give equal bytes.  No kernel waits for another work-group.
 *   CCLIP_ERR_ARG, nothing launched, nothing written: pred, gt, confusion or bad NULL; C outside [1, 255]; band outside
 *   [0, CCLIP_AGREEMENT_MAX_BAND]; bands given with band == 0 or missing with band > 0; per_image or accumulate other than 0 or
 *   1; B < 1; H or W outside [1, CCLIP_OVERLAY_MAX_SIDE]; B H W > 2^31 - 1 (formed in 64 bits); confusion, bad or bands not
 *   8-byte aligned; an output that overlaps another output or an input.  pred and gt may have any alignment.
 *   While C (C + 1) <= CCLIP_AGREEMENT_HIST_CELLS (C <= 44) the confusion counts of a tile are gathered in LDS. */
#define CCLIP_AGREEMENT_MAX_BAND 32
#define CCLIP_AGREEMENT_HIST_CELLS 2048
int cclip_label_agreement(const uint8_t* pred, const uint8_t* gt, int32_t B, int32_t H, int32_t W, int32_t C, int32_t band,
                          int32_t per_image, int32_t accumulate, int64_t* confusion, int64_t* bad, int64_t* bands,
                          hipStream_t stream);

/* cclip_dense_prototypes (csrc/dense_prototypes.hip): few-shot class prototypes for the dense path by masked average pooling.
 *   The per-patch features of K windows are pooled under annotated masks into one weighted sum per class; fp32, no fp16 twin.
 *     feat   fp32 [K g g][E], row stride ldf (floats): window k owns rows k g g .. k g g + g g - 1, row i g + j is cell (row i,
 *            column j) - encode_image_dense viewed flat, as cclip_dense_class_probs takes it
 *     masks  uint8 [B][H][W]: class indices < C; 255 = ignore; values in [C, 254] are "bad"
 *     boxes  int32 [K][4] = (x0, y0, x1, y1), on the device;  image int32 [K] on the device, or NULL = every window is of image 0
 *   Window validity: 1 <= x1 - x0 <= CCLIP_OVERLAY_MAX_SIDE and 1 <= y1 - y0 <= CCLIP_OVERLAY_MAX_SIDE, the sides formed without
 *     32-bit overflow, and 0 <= image[k] < B.  Any other window contributes nothing; a box may hang over the picture's edge.  The
 *     launcher cannot see boxes or image: for ANY values in them the kernel reads nothing outside its inputs and writes nothing
 *     outside its outputs and workspace.
 *   Cells: pixel (x, y) of a valid window lies in cell column j = ((2 (x - x0) + 1) g) / (2 (x1 - x0)) and row i likewise from y
 *     (integer division, the pixel-centre rule, consistent with the align_corners=False geometry of cclip_dense_stitch).
 *     area(k,i,j) = the box pixels in the cell, inside the picture or not; count_c(k,i,j) = those of them inside the picture with
 *     mask == c < C.  A side shorter than g leaves cells with area == 0, which contribute nothing.
 *   Contribution: a cell contributes to class c when count_c > 0 and 256 count_c >= min_share8 area (64-bit products; min_share8 in
 *     [0, 256], the a8 idiom: 256 = only cells wholly of one class, 0 = any overlap), with weight w = (float)count_c / (float)area,
 *     one fp32 division.  f^_p = feat_p / |feat_p|, the zero vector when the norm is 0 (no epsilon, cclip_dense_class_probs's
 *     rule; the cell still counts in patches).
 *   Outputs - accumulate == 0 sets them, accumulate == 1 adds to what they hold (one fp32 add per float element, integer adds):
 *     sums    fp32  [C][E] = the sum over contributing cells of w f^        weight  fp32 [C] = the sum of w
 *     patches int64 [C]    = the number of contributing cells
 *     pixels  int64 [C]    = the sum of count_c over ALL cells of all valid windows (a pixel under two windows counts twice;
 *                            cells below the threshold count as well)
 *     bad     int64 [1]    = pixels inside the picture and inside a valid window with a mask value in [C, 254]
 *     A class that nothing contributes to gets sums exactly 0, weight 0 and patches 0.
 *   Determinism: the K g g cells are cut into slabs of CCLIP_PROTOTYPES_SLAB consecutive cells, a function of K and g alone; one
 *     work-group walks a slab in ascending cell order into its own partial, a second kernel adds the slabs in ascending order.
 *     No float atomics (integer atomics for the counts), nothing depends on the device or the launch geometry: two calls give
 *     equal bytes.
 *   workspace: 16-byte aligned, at least cclip_dense_prototypes_workspace(K, g, C, E) bytes =
 *     ceil(K g g / CCLIP_PROTOTYPES_SLAB) * C * (E + 2) * 4   (per slab and class: E partial sums, a weight, a patch count).
 *   CCLIP_ERR_ARG, nothing launched, nothing written: a NULL pointer other than image; K outside [1, 65535]; C outside [1, 255];
 *   g, H or W outside [1, CCLIP_OVERLAY_MAX_SIDE]; B < 1; B H W > 2^31 - 1 (formed in 64 bits); E outside [4, 1024] or not a
 *   multiple of 4; ldf < E or not a multiple of 4; K g g ldf > 2^62 (row indices stay inside 64 bits); feat or workspace not 16-byte aligned; sums, weight, boxes or image not 4-byte
 *   aligned; patches, pixels or bad not 8-byte aligned; min_share8 outside [0, 256]; accumulate other than 0 or 1; a workspace
 *   that is too small; an output (the workspace is one) that overlaps another output or an input.  masks may have any alignment. */
#define CCLIP_PROTOTYPES_SLAB 64
int64_t cclip_dense_prototypes_workspace(int32_t K, int32_t g, int32_t C, int32_t E);
int cclip_dense_prototypes(const float* feat, int64_t ldf, const uint8_t* masks, const int32_t* boxes, const int32_t* image,
                           int32_t K, int32_t g, int32_t C, int32_t E, int32_t B, int32_t H, int32_t W, int32_t min_share8,
                           int32_t accumulate, float* sums, float* weight, int64_t* patches, int64_t* pixels, int64_t* bad,
                           void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* ---- CLIP-guided caption selection ---------------------------------------------------------------
 * K candidate captions for each of N images, scored against the image (CLIPScore, Hessel et al. 2021), optionally against the
 * image's reference captions (RefCLIPScore), and ranked - one launch, one work-group per image (csrc/caption_select.hip).
 * Every buffer is fp32 (the towers' outputs after .float(), raw, not normalised); there is no fp16 twin.
 *   img [N][E] row stride ldi; txt [N*K][E] row stride ldt, row n*K + k = candidate k of image n;
 *   lm_mean [N*K] or NULL (= 0): the mean token log-probability of the candidate;
 *   ref [Rtot][E] row stride ldr with CSR offsets ref_off int32 [N+1] (image n owns rows ref_off[n] .. ref_off[n+1]-1; an
 *   image may own none), both NULL = no RefCLIPScore (ref_score is then not touched and may be NULL).
 *   cos[n][k]   = <i_n, t_nk> / (|i_n| |t_nk|), 0 when either norm is 0
 *   clip_score  = w * max(cos, 0)
 *   rmax[n][k]  = max(0, max_r cos(t_nk, ref_r)) over image n's references, 0 when it has none
 *   ref_score   = 2 * clip_score * rmax / (clip_score + rmax), 0 when the denominator is 0
 *   score       = cos + lm_weight * lm_mean
 *   order[n][:] = the candidates by (score descending, k ascending), int32;  best[n] = order[n][0]
 * Scores are compared through a monotone integer image of their fp32 bits (-0 == +0): order[n][:] is a permutation of
 * 0 .. K-1 for any input, NaN included.  Values from non-finite features are otherwise undefined; no access leaves the buffers.
 * |cos - exact| <= 4 (E/64 + 8) 2^-24.  No atomics: two calls agree bit for bit, and a row's results do not depend on N.
 * CCLIP_ERR_ARG, nothing launched: a required pointer NULL; N <= 0; K < 1 or K > CCLIP_CAPTION_SELECT_MAX_K; E <= 0, E % 4 != 0
 * or E > CCLIP_CAPTION_SELECT_MAX_E; a stride below E or not a multiple of 4; img / txt / ref not 16-byte aligned; ref without
 * ref_off or ref_off without ref.  ref_off is read on the device only: a decreasing or out-of-bounds range is the caller's
 * error (the Python layer validates the offsets on the host before upload). */
#define CCLIP_CAPTION_SELECT_MAX_K 64
#define CCLIP_CAPTION_SELECT_MAX_E 1024
int cclip_caption_select(const float* img, int64_t ldi, const float* txt, int64_t ldt, int32_t N, int32_t K, int32_t E,
                         const float* lm_mean, const float* ref, int64_t ldr, const int32_t* ref_off, float w, float lm_weight,
                         float* cos, float* clip_score, float* ref_score, float* score, int32_t* order, int32_t* best,
                         hipStream_t stream);

/* ---- IEEE fp16 twins ---------------------------------------------------------------------------
 * Every entry point above whose 16-bit buffers are bf16 has a twin with the identical signature that
 * treats them as IEEE fp16 (same MFMA rate on gfx950; 3 more mantissa bits - the reference's own CUDA
 * dtype, and the mode in which the towers meet the <= 1e-3 parity target; use bf16 for training range). */
int cclip_gemm_f16(const cclip_gemm_desc* d, hipStream_t stream);
int cclip_layernorm_fwd_f16(const float* x, int64_t ldx, const int32_t* row_index, int32_t rows, int32_t D,
                            const float* gamma, const float* beta, float eps, void* out_f16, float* out_f32,
                            int64_t ldo, float* mean, float* rstd, hipStream_t stream);
int cclip_layernorm_bwd_f16(const void* dy, int32_t dy_is_f16, int64_t lddy, const float* x, int64_t ldx,
                            const int32_t* row_index, int32_t rows, int32_t D, const float* gamma,
                            const float* mean, const float* rstd, const float* dx_res, float* dx_out,
                            void* dx_out_f16, int64_t lddx, float* dgamma, float* dbeta, int32_t accumulate,
                            float* ws, hipStream_t stream);
int cclip_attention_fwd_f16(const cclip_attn_desc* d, hipStream_t stream);
int cclip_attention_bwd_f16(const cclip_attn_desc* d, hipStream_t stream);
int cclip_attention_relevance_f16(const cclip_attn_desc* d, float grad_scale, float* R, hipStream_t stream);
int cclip_attention_relevance_row_f16(const cclip_attn_desc* d, float grad_scale, const float* r_in, float* r_out,
                                      hipStream_t stream);
int cclip_attention_probs_f16(const cclip_attn_desc* d, const int32_t* q_rows, int32_t n_q, float* P, int64_t ld_p_b,
                              int64_t ld_p_h, int64_t ld_p_q, hipStream_t stream);
int cclip_attention_small_fwd_f16(const cclip_attn_desc* d, hipStream_t stream);
int cclip_attention_small_bwd_f16(const cclip_attn_desc* d, hipStream_t stream);
int cclip_attention_decode_f16(const void* q, int64_t ldq, const void* kcache, const void* vcache, int64_t ld_pos,
                               int64_t ld_seq, void* out, int64_t ldo, int32_t B, int32_t H, int32_t S, float scale,
                               hipStream_t stream);
int cclip_patchify_f16(const float* image, void* out_f16, int32_t B, int32_t R, int32_t P, hipStream_t stream);
int cclip_colsum_f16(const void* in, int32_t in_is_f16, int64_t ld, int32_t R, int32_t C, float* out,
                     int32_t accumulate, float* ws, hipStream_t stream);
int cclip_xent_rows_f16(const float* logits, int64_t ld, int32_t R, int32_t C, const int32_t* labels,
                        int32_t ignore_index, float grad_scale, float* loss_row, int32_t* pred,
                        void* dlogits, int32_t dlogits_is_f16, int64_t ldd, float* rowdot, hipStream_t stream);
int cclip_gpt2_decode_step_f16(const cclip_decode_desc* d, hipStream_t stream);
int cclip_gpt2_beam_search_f16(const cclip_beam_desc* d, hipStream_t stream);
int cclip_gpt2_beam_search_batch_f16(const cclip_beam_batch_desc* d, hipStream_t stream);
int cclip_quantize_rows_fp8_f16(const void* x_f16, int64_t ldx, int32_t rows, int32_t cols, void* out_fp8, int64_t ldo,
                                float* scale, hipStream_t stream);
int cclip_gemm_fp8_f16(const void* A8, int64_t lda, const float* scale_a, const void* B8, int64_t ldb, const float* scale_b,
                       int32_t M, int32_t N, int32_t K, const float* bias, int32_t act, void* out_f16, int64_t ldc,
                       hipStream_t stream);
int cclip_quantize_mx_fp8_f16(const void* x_f16, int64_t ldx, int32_t rows, int32_t cols, void* out_fp8, int64_t ldo,
                              void* block_scale, int64_t ld_block_scale, hipStream_t stream);
int cclip_gemm_fp8_ex_f16(const cclip_fp8_gemm_desc* d, hipStream_t stream);
int cclip_adamw_step_f16(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                         float beta1, float beta2, float eps, float weight_decay, int32_t step,
                         int32_t correct_bias, float grad_scale, int32_t mode, void* f16_shadow,
                         hipStream_t stream);
int cclip_adamw_step_groups_f16(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                const uint8_t* chunk_group, const float* lr, const float* weight_decay, int32_t n_groups,
                                float beta1, float beta2, float eps, int32_t step, int32_t correct_bias, float grad_scale,
                                int32_t mode, void* f16_shadow, const float* sumsq_dev, float max_norm, int32_t skip_nonfinite,
                                float* ema, float ema_decay, hipStream_t stream);
int cclip_cast_f32_to_f16(const float* in, void* out, int64_t n, hipStream_t stream);
int cclip_similarity_topk_f16(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                              int32_t k, float* scores, int32_t* index, void* workspace, int64_t workspace_bytes,
                              hipStream_t stream);
int cclip_similarity_topk_biased_f16(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                                     int32_t k, const float* bias, float scale, float* scores, int32_t* index, void* workspace,
                                     int64_t workspace_bytes, hipStream_t stream);
int cclip_bank_lse_f16(const void* g, int64_t ldg, int64_t N, const void* bank, int64_t ldb, int64_t B, int32_t D, float beta,
                       float* lse, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_similarity_range_count_f16(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                                     float threshold, int32_t self_join, int32_t* counts, int64_t workspace_bytes,
                                     hipStream_t stream);
int cclip_similarity_range_emit_f16(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t N, int32_t D,
                                    float threshold, int32_t self_join, const int64_t* starts, int64_t total, int64_t H,
                                    int32_t* index, float* scores, hipStream_t stream);
int cclip_lm_head_score_f16(const void* x, int64_t ldx, int32_t R, int32_t D, const void* w, int64_t ldw, int32_t V,
                            const int32_t* labels, int32_t ignore_index, float* logp, float* lse, int32_t* pred,
                            float* pred_logit, void* workspace, hipStream_t stream);
int cclip_cache_affinity_f16(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t Np, int32_t D,
                             const int32_t* class_off, const int32_t* class_len, int32_t C, float beta, const int32_t* exclude,
                             float* out, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_cache_affinity_bwd_f16(const void* q, int64_t ldq, int32_t Q, const void* g, int64_t ldg, int64_t Np, int32_t D,
                                 const int32_t* class_off, const int32_t* class_len, int32_t C, float beta,
                                 const int32_t* exclude, const float* dA, float* dG, void* workspace, int64_t workspace_bytes,
                                 hipStream_t stream);
int cclip_kmeans_assign_f16(const void* x, int64_t ldx, int64_t N, const void* c, int64_t ldc, int64_t K, int32_t D,
                            int32_t* assign, float* best, float* second, hipStream_t stream);
int cclip_kmeans_update_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const int32_t* order, const int32_t* seg_off,
                            int64_t K, const void* prev_c, int64_t ldp, void* out_c, int64_t ldo, float* out_norm,
                            void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_coreset_step_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const float* weight, float* mind, int32_t* owner,
                           int32_t centre, const void* partial_in, void* partial_out, int32_t* pick_out, float* radius_out,
                           hipStream_t stream);
int cclip_coreset_greedy_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const float* weight, float* mind, int32_t* owner,
                             int32_t first, int64_t m, int32_t* picks, float* radius, void* workspace, int64_t workspace_bytes,
                             hipStream_t stream);
int cclip_mreach_nearest_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const float* core, const int32_t* comp,
                             void* keys, hipStream_t stream);
int cclip_mst_boruvka_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const float* core, int32_t* u, int32_t* v, float* m,
                          void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_probe_forward_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const float* W, const float* bias, int32_t C,
                            const int32_t* labels, const float* row_weight, float* lse, float* loss, int32_t* pred,
                            float* logits, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_probe_backward_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const float* W, const float* bias, int32_t C,
                             const int32_t* labels, const float* row_weight, const float* lse, const float* loss, float scale,
                             float l2, float* dW, float* db, float* objective, void* workspace, int64_t workspace_bytes,
                             hipStream_t stream);
int cclip_concept_codes_f16(const void* x, int64_t ldx, int64_t N, const void* c, int64_t ldc, int64_t V, int32_t D, float l1,
                            float eta, int32_t iters, float* w, int64_t ldw, float* resid2, float* l1norm, int32_t* nnz,
                            float* delta, float* kkt, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_class_moments_f16(const void* x, int64_t ldx, int64_t N, int32_t D, const int32_t* labels, int32_t C, int32_t* count,
                            float* sum, float* gram, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cclip_gauss_scores_f16(const void* x, int64_t ldx, int64_t Q, int32_t D, const float* T, const float* t0, int32_t R,
                           const float* centres, const float* offset, int32_t C, int32_t* pred, float* lse, int32_t* nearest,
                           float* dmin, float* d2, float* z, void* workspace, int64_t workspace_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CCLIP_HIP_H */
