/* llx.h - C ABI of libllx_hip.so: the MI355X (gfx950) kernels behind the llama-x training hot path.
 *
 * Drop-in boundary: the reference (gau-nernst/llama-x) is pure Python and reaches the
 * device through PyTorch / Triton calls inside its `modelling` and `subclasses` packages.  This library is what the
 * Python side of those packages binds (ctypes) instead; each entry point names the reference call site it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *   - bf16 tensors are passed as `const void*` to raw 16-bit storage, row-major, last dimension contiguous;
 *     `ld*` / `*_ss` / `*_sb` are strides in ELEMENTS;
 *   - the caller owns every buffer (PyTorch's caching allocator); the library never allocates, frees, retains or
 *     synchronises; workspaces are caller-provided (size queries are host functions);
 *   - every launcher takes the stream to launch on (`hipStream_t`, passed as void* from ctypes) and is re-entrant;
 *   - return value 0 = success; negative = error (-1 bad argument, -2 launch failure, -3 unsupported); the message is
 *     in llx_last_error_string() (thread-local).  No exceptions, no abort.
 */
#ifndef LLX_H
#define LLX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* llx_stream_t; /* hipStream_t */

/* ---- library ------------------------------------------------------------------------------------------------ */
int llx_version(void);                                   /* 105 = 0.1.5 */
const char* llx_last_error_string(void);                 /* thread-local, valid until the next failing call */
int llx_device_info(int device, char* name, int len);    /* returns CU count, fills gcn arch name */

/* ---- RMSNorm: nn.RMSNorm(D, eps=1e-5) at modelling/llama.py:158,160,182 (called :172,173,216) ----------------- */
int llx_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t dim, float eps, llx_stream_t s);
/* the same, also emitting quantize_int8_rowwise(y) (q int8 [rows,dim], row stride ldq; qscale bf16 [rows]) for the dynamic-int8-activation
 * linears that follow the norm (subclasses/int8.py:110-113): bit-identical to llx_quantize_int8_rowwise on y, one pass */
int llx_rmsnorm_fwd_quant(const void* x, const void* w, void* y, float* rstd, void* q, int64_t ldq, void* qscale, int64_t rows, int64_t dim,
                          float eps, llx_stream_t s);
int64_t llx_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t dim);
int llx_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx, void* dw /*nullable*/,
                    int dw_accumulate, void* workspace, const void* dres /*nullable: residual-branch gradient added to dx*/,
                    int64_t rows, int64_t dim, llx_stream_t s);

/* ---- bf16 MFMA GEMM, C[M,N] = A[M,K].B[N,K]^T (+ A2[M,K2].B2[N,K2]^T): every F.linear of the layer
 *      (modelling/llama.py:118-120,140,152,216), its data gradients (on a transposed weight image), the LoRA adapter
 *      as K-extension (modelling/lora.py:43) and the audio convolutions as implicit GEMMs (modelling/audio.py:26-31).
 *      epilogue: 0 none | 1 + E[M,N] (ld = lde) | 2 + bias E[N] | 3 gelu(+bias E[N]) | 4 * colscale E[N]
 *      (weight-only int8, subclasses/int8.py:118) | 6 SwiGLU backward: the product is dh = dL/d(silu(g)*u) of the feed-forward
 *      (modelling/llama.py:150); E = gate|up activations [M,2N], C = dg|du [M,2N], dh is not stored.
 *      | 7 SwiGLU forward: B = [W_gate; W_up] (N = 2I, I % 128 == 0), C = gate|up [M,N] as usual, E = OUTPUT h [M,I] = silu(g)*u
 *      (row stride lde); a tile covers 128 gate columns and the matching 128 up columns.
 *      K, K2 multiples of 64; N multiple of 8. ------------------------------------------------------------------- */
int llx_gemm_nt_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                     const void* A2, int64_t lda2, const void* B2, int64_t ldb2, int64_t K2, int epilogue, const void* E, int64_t lde,
                     llx_stream_t s);
/* llx_gemm_nt_bf16 over the first *m_valid rows only (m_valid: DEVICE int32, read by the kernel, so the launch is capturable): row
 * tiles of 256 that start at or after *m_valid are skipped, rows of C from *m_valid to the end of that tile are computed from
 * whatever A holds there.  The LM head of modelling/llama.py:216-218 over the positions whose label is not ignore_index. */
int llx_gemm_nt_bf16_rows(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          const void* A2, int64_t lda2, const void* B2, int64_t ldb2, int64_t K2, int epilogue, const void* E, int64_t lde,
                          const int32_t* m_valid, llx_stream_t s);
/* Split-K form for a product with few output tiles and a long contraction (d hidden = d logits . W of the LM head, modelling/llama.py:216:
 * 16 x 16 tiles, K = 128256): partial[s][M][N] fp32 (row stride N) for `splits` equal K ranges from ONE launch over (range, row tile,
 * column tile); m_valid (nullable) as in llx_gemm_nt_bf16_rows.  K % (64 * splits) == 0.
 * llx_splitk_combine: out[i] = bf16(scale[0] * bf16(sum_s partial[s][inv ? inv[i] : i])), zero rows where inv[i] < 0 (inv, scale nullable). */
int llx_gemm_nt_bf16_splitk(const void* A, int64_t lda, const void* B, int64_t ldb, float* partial, int64_t M, int64_t N, int64_t K, int splits,
                            const int32_t* m_valid, llx_stream_t s);
int llx_splitk_combine(const float* partial, int splits, int64_t M, int64_t N, const int32_t* inv, const float* scale, void* out, int64_t ld_out,
                       llx_stream_t s);
/* The q|k|v projection with apply_rope (modelling/llama.py:118-125, 63-73) in the epilogue: columns [0, rope_cols) of C (whole
 * 128-wide heads: q then k) are rotated with the fp32 table [>= rope_S, 64, 2]; row m of C is sequence position m % rope_S.
 * Bit-identical to llx_gemm_nt_bf16(epilogue 0) followed by llx_rope. */
int llx_gemm_nt_bf16_rope(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          const void* A2, int64_t lda2, const void* B2, int64_t ldb2, int64_t K2, const float* rope_table, int64_t rope_S,
                          int64_t rope_cols, llx_stream_t s);

/* ---- the weight gradient of a dense linear, dW[out,in] = dy[T,out]^T . x[T,in] (autograd of F.linear for the weights the scripts leave
 *      trainable: tok_embeddings / norm / output by default, train_metamathqa.py:177-180; the Conv1d weights of modelling/audio.py:26-31 as
 *      an implicit GEMM): C[N1,N2] = A[M,N1]^T . B[M,N2], operands read as they lie (token-major rows, row-strided views allowed), no
 *      transposed copies.  N1, N2 multiples of 8; any M. ------------------------------------------------------------------------------- */
int llx_gemm_tn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N1, int64_t N2,
                     llx_stream_t s);
/* ... over the first min(M, *m_valid) rows only (m_valid: device int32, nullable): the weight gradient of a trainable LM head over the
 * compacted labelled rows - F.cross_entropy's ignore_index rows have zero gradient rows (modelling/llama.py:216-218). */
int llx_gemm_tn_bf16_rows(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N1, int64_t N2,
                          const int32_t* m_valid, llx_stream_t s);

/* ---- torchao::int8_mm_dequant(A, B, A_scale, B_scale) - subclasses/int8_mm.py:121-149 (Triton kernel :50-118).
 *      A int8 [M,K]; B passed as its K-contiguous rows [N,K] (= the reference's int_data.T view, strides (1,K));
 *      scales bf16; C bf16 = (int32 acc) * a_scale[m] * b_scale[n], one rounding.  K multiple of 128. ----------- */
int llx_int8_mm_dequant(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                        const void* a_scale, const void* b_scale, llx_stream_t s);
/* fp32 scales -> fp32 C (the op returns dtype = A_scale.dtype: subclasses/int8_mm.py:126,136,143); ldc in fp32 elements. */
int llx_int8_mm_dequant_f32(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                            const float* a_scale, const float* b_scale, llx_stream_t s);
/* The same with the neighbours of its call sites fused in (int8 base, dynamically quantised activations - subclasses/int8.py:110-118):
 * C = epilogue( bf16( bf16(int8_mm_dequant(A, B, a_scale, b_scale)) + A2[M,K2].B2[N,K2]^T ) ).  A2/B2 (nullable; bf16, K2 % 64 == 0):
 * the LoRA adapter (modelling/lora.py:43) - the int32 accumulators are dequantised in place, the extension accumulates on top in fp32.
 * epilogue: 0 none | 1 + E[M,N] (ld = lde) | 7 SwiGLU forward (E = OUTPUT h) | 8 RoPE on columns [0, rope_cols), as llx_gemm_nt_bf16(_rope). */
int llx_int8_mm_dequant_ext(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                            const void* a_scale, const void* b_scale, const void* A2, int64_t lda2, const void* B2, int64_t ldb2, int64_t K2,
                            int epilogue, const void* E, int64_t lde, const float* rope_table, int64_t rope_S, int64_t rope_cols,
                            llx_stream_t s);

/* ---- quantize_int8_rowwise - subclasses/int8.py:10-16 (weights once, activations per forward when dynamic). ---- */
int llx_quantize_int8_rowwise(const void* x, int64_t ldx, void* q, int64_t ldq, void* scale, int64_t rows, int64_t cols, int is_f32,
                              llx_stream_t s);

/* ---- attention: F.scaled_dot_product_attention(..., enable_gqa=True) and flex_attention(block_mask=...) at
 *      modelling/llama.py:129-137; mask rule = mask_mod of train_metamathqa.py:67-68 plus the prefix-LM term
 *      (README.md:16): allow(q,k) = (k <= q || k < prefix_len[b]) && (!doc_ids || doc_ids[b,q] == doc_ids[b,k]).
 *      q [B,S,H,128], k/v [B,S,KVH,128] with free batch/sequence strides; lse fp32 [B,H,S] (log2 units).
 *      flags: tile classes built by llx_attn_tile_flags (needed only with doc_ids / prefix_len). ----------------- */
int64_t llx_attn_flags_bytes(int64_t B, int64_t S);
int llx_attn_tile_flags(const int* doc_ids, const int* prefix_len, void* flags, int64_t B, int64_t S, llx_stream_t s);
int llx_attn_fwd(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss, const void* v, int64_t v_sb,
                 int64_t v_ss, void* o, int64_t o_sb, int64_t o_ss, float* lse, const int* doc_ids, const int* prefix_len,
                 const void* flags, int64_t B, int64_t S, int64_t H, int64_t KVH, int64_t head_dim, float scale, llx_stream_t s);
int64_t llx_attn_bwd_workspace_bytes(int64_t B, int64_t S, int64_t H, int64_t KVH); /* delta + per-head dK/dV partials */
int64_t llx_attn_bwd_ds_bytes(int64_t B, int64_t S, int64_t H); /* optional bf16 dS^T scratch [B,H,Sp,Sp], Sp = S rounded up to 256 */
int llx_attn_bwd(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss, const void* v, int64_t v_sb,
                 int64_t v_ss, const void* o, int64_t o_sb, int64_t o_ss, const void* d_o, int64_t do_sb, int64_t do_ss, const float* lse,
                 float* delta /* fp32 workspace, llx_attn_bwd_workspace_bytes() */, void* dq, int64_t dq_sb, int64_t dq_ss, void* dk, int64_t dk_sb, int64_t dk_ss,
                 void* dv, int64_t dv_sb, int64_t dv_ss, const int* doc_ids, const int* prefix_len, const void* flags,
                 const float* rope /* nullable fp32 [>=S,64,2]: dq, dk leave already multiplied by apply_rope's transpose */,
                 void* ds /* nullable scratch of llx_attn_bwd_ds_bytes(): dS^T makes one round trip through it and each of the five products
                             (S, dP, dV, dK, dQ) is computed once; without it the dQ kernel recomputes S and dP */,
                 int64_t B, int64_t S, int64_t H, int64_t KVH, int64_t head_dim, float scale, llx_stream_t s);

/* ---- attention dropout in training: F.scaled_dot_product_attention(..., dropout_p) at modelling/llama.py:135-137.  The two entries
 *      above with three more operands in front of the stream: threshold = t = round(p * 65536), 0 < t < 65536 (an element is dropped with
 *      probability t / 65536, a kept one is scaled by 65536 / (65536 - t)); rng = device pointer to two int64 (seed, counter), read by
 *      the kernels - the backward must see the values the forward saw, so callers hand both a per-step copy (the ticket) of their live
 *      state; stream_id = one value per attention module.  keep(b, h, q, k) is a counter-based integer hash of (seed, counter, stream_id,
 *      b, h, q, k) (csrc/attn_dropout.h), independent per QUERY head.  The softmax statistics and lse are those of the undropped rows;
 *      O = sum_k (P keep c) V, dV = (P keep c)^T dO, dP = keep c (dO V^T), dS = P (dP - delta).  llx_attn_bwd_dropout takes ds = null
 *      only (the dS scratch route has no dropout build).  llx_attn_dropout_keep writes the keep bytes [B, H, Sq, Skv] (1 = kept). ---- */
int llx_attn_fwd_dropout(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss, const void* v, int64_t v_sb,
                         int64_t v_ss, void* o, int64_t o_sb, int64_t o_ss, float* lse, const int* doc_ids, const int* prefix_len,
                         const void* flags, int64_t B, int64_t S, int64_t H, int64_t KVH, int64_t head_dim, float scale, int64_t threshold,
                         const void* rng, int64_t stream_id, llx_stream_t s);
int llx_attn_bwd_dropout(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss, const void* v, int64_t v_sb,
                         int64_t v_ss, const void* o, int64_t o_sb, int64_t o_ss, const void* d_o, int64_t do_sb, int64_t do_ss,
                         const float* lse, float* delta, void* dq, int64_t dq_sb, int64_t dq_ss, void* dk, int64_t dk_sb, int64_t dk_ss,
                         void* dv, int64_t dv_sb, int64_t dv_ss, const int* doc_ids, const int* prefix_len, const void* flags,
                         const float* rope, void* ds, int64_t B, int64_t S, int64_t H, int64_t KVH, int64_t head_dim, float scale,
                         int64_t threshold, const void* rng, int64_t stream_id, llx_stream_t s);
int llx_attn_dropout_keep(void* keep, int64_t B, int64_t H, int64_t Sq, int64_t Skv, int64_t threshold, const void* rng, int64_t stream_id,
                          llx_stream_t s);

/* ---- dense-mask attention forward (inference / KV-cache path): SDPA(q,k,v,mask,is_causal=False,enable_gqa=True) at
 *      modelling/llama.py:126-127,135-137 with mask = causal_mask[None,None,input_pos] (:194,:205).  q [B,H,Sq,128],
 *      k/v [B,KVH,Skv,128] (e.g. the KVCache buffers :79-81), mask bool with broadcast strides; forward only. ------- */
int llx_attn_dense_fwd(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                       const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, void* o, int64_t o_sb, int64_t o_sh, int64_t o_ss,
                       const void* mask, int64_t m_sb, int64_t m_sh, int64_t m_sq, int64_t B, int64_t H, int64_t KVH, int64_t Sq, int64_t Skv,
                       int64_t head_dim, float scale, llx_stream_t s);

/* ---- the same SDPA call (modelling/llama.py:126-127,135-137 with the mask of :194,:205) for a mask broadcast over heads, on the MFMA
 *      tile loop of llx_attn_fwd: KV-cache prefill and explicit bool masks.  Sq query rows against Skv keys; the mask is the only rule.
 *      q / o are ROWS [B, Sq, H*128] (batch / position strides, head h at h*128; o is what wo reads), k / v [B, KVH, Skv, 128] through
 *      (batch, head, position) strides - the cache buffers or the views of a fused q|k|v row buffer.  mask bool / uint8 [B | 1, Sq, Skv],
 *      last dim dense, m_sq / m_sb in bytes (m_sb = 0 broadcasts), Skv >= 4.  flags: llx_attn_mask_flags_bytes(B, Sq, Skv) bytes filled
 *      by llx_attn_mask_tile_flags (128-row x 64-key tile classes: 0 skipped, 1 tested per byte, 2 unmasked).  lse nullable (fp32
 *      [B,H,Sq], log2 units).  A row without any allowed key comes out NaN, as SDPA's.  Backward: llx_attn_mask_bwd (Sq = Skv). --- */
int64_t llx_attn_mask_flags_bytes(int64_t B, int64_t Sq, int64_t Skv);
int llx_attn_mask_tile_flags(const void* mask, int64_t m_sb, int64_t m_sq, void* flags, int64_t B, int64_t Sq, int64_t Skv, llx_stream_t s);
int llx_attn_mask_fwd(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v,
                      int64_t v_sb, int64_t v_sh, int64_t v_ss, void* o, int64_t o_sb, int64_t o_ss, float* lse /* nullable */,
                      const void* mask, int64_t m_sb, int64_t m_sq, const void* flags, int64_t B, int64_t Sq, int64_t Skv, int64_t H,
                      int64_t KVH, int64_t head_dim, float scale, llx_stream_t s);

/* ---- training through any bool mask: the gradients autograd produces for the same SDPA call with an arbitrary dense mask, and for
 *      flex_attention with a BlockMask of an arbitrary mask_mod (modelling/llama.py:129-137), with Sq = Skv = S.  Everything as
 *      llx_attn_bwd (rows [B,S,H|KVH,128] with batch / sequence strides in elements, lse as llx_attn_mask_fwd wrote it, the workspace of
 *      llx_attn_bwd_workspace_bytes(), nullable rope) except the rule: mask / m_sb / m_sq / flags as in llx_attn_mask_fwd with
 *      flags = llx_attn_mask_tile_flags(mask, .., B, S, S); S >= 4.  Nothing causal is assumed: tiles above the diagonal can be live, and
 *      a key that no row attends to gets exact zeros in dk / dv.  A row without any allowed key (NaN in the forward) has meaningless
 *      gradients, as in the reference; the kernels stay memory-safe on it.  Deterministic (no atomics). ---------------------------- */
int llx_attn_mask_bwd(const void* q, int64_t q_sb, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_ss, const void* v, int64_t v_sb,
                      int64_t v_ss, const void* o, int64_t o_sb, int64_t o_ss, const void* d_o, int64_t do_sb, int64_t do_ss,
                      const float* lse, float* delta /* fp32 workspace, llx_attn_bwd_workspace_bytes() */, void* dq, int64_t dq_sb,
                      int64_t dq_ss, void* dk, int64_t dk_sb, int64_t dk_ss, void* dv, int64_t dv_sb, int64_t dv_ss, const void* mask,
                      int64_t m_sb, int64_t m_sq, const void* flags, const float* rope /* nullable, as in llx_attn_bwd */, int64_t B,
                      int64_t S, int64_t H, int64_t KVH, int64_t head_dim, float scale, llx_stream_t s);

/* ---- decode path: a few query tokens (M <= 4) against the KV cache - modelling/llama.py:76-90 (KVCache), :126-127,:135-137 (cached
 *      K/V through SDPA with the row-gathered causal mask), :189-194,:205-207 (Llama.forward with input_pos).  Every linear is a
 *      weight stream: all CUs read weight rows once (llx_gemv_bf16), the call sites' neighbours ride in its prologue / epilogue. ---- */
/* out = epilogue( [rmsnorm(x) | x][M, K] . [W0; W1; W2]^T ): F.linear at modelling/llama.py:118-120,140,152,216 for M <= 4 rows.
 * W_s [n_s, K] bf16 row-major (ld = ldw_s; w1 / w2 nullable with n = 0; inner n_s % 4 == 0), K % 8 == 0; norm_w (nullable): nn.RMSNorm
 * (:158-160,182) applied to x first.  epilogue 0: out [M, N] | 1: + res [M, N] (:172-173) | 2 (q|k|v): apply_rope (:63-73,122-123;
 * table row = token index in this call, :207) on rows [0, n_q) -> out [M, n_q] and on rows [n_q, n_q + n_k) -> k cache, remaining
 * rows -> v cache, both at input_pos[m] (device int64; KVCache.update :83-90; caches [KVH, Smax, 128] through (head, position)
 * strides) | 3 (gate|up: W0, W1, N = 2 n_0): out [M, n_0] = silu(gate) * up (:150-152).  LoRA (modelling/lora.py:43; bext_s
 * [n_s, rank_s] nullable, t [M, sum rank] bf16 = x . A^T from a previous call, rank % 8 == 0): out += lora_scale * t_s . bext_s[row]. */
int llx_gemv_bf16(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2, int64_t n2,
                  const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out, int64_t ldo,
                  const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache, int64_t c_sh,
                  int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1, const void* bext2, int64_t rank0, int64_t rank1,
                  int64_t rank2, const void* t, int64_t ldt, float lora_scale, llx_stream_t s);
/* llx_gemv_bf16 on int8 weight rows: F.linear on an Int8LinearWeight (subclasses/int8.py:106-121) at the same call sites of a model
 * after quantize_linear_(model.layers, "int8", ...).  W_s [n_s, K] int8 row-major (ldw_s in bytes, % 16), scale_s [n_s] bf16 per-row
 * scales, K % 16 == 0, all members of a call of one kind.  dynamic = 0 (weight-only, :118): out = bf16(bf16(x . W^T) * scale[row]).
 * dynamic = 1 (:112-113, int8_mm.py:93-118): each (normalised) row of x is quantised as llx_quantize_int8_rowwise does, int32 dot
 * products, out = bf16(((float)acc * x_scale[m]) * scale[row]) - bit-exact with the reference when no norm is fused.  Norm, epilogues
 * and LoRA operands as llx_gemv_bf16 (t = x . A^T from llx_gemv_bf16 on the un-quantised x): out = bf16(out + lora_scale * t_s . bext_s[row]). */
int llx_gemv_i8(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2, int64_t n2,
                const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out, int64_t ldo,
                const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache, int64_t c_sh,
                int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1, const void* bext2, int64_t rank0, int64_t rank1,
                int64_t rank2, const void* t, int64_t ldt, float lora_scale, const void* scale0, const void* scale1, const void* scale2,
                int dynamic, llx_stream_t s);
/* llx_gemv_bf16 on DoRA linears (modelling/lora.py:51-59) whose row factor c_s = m / ||W_s + s B_s A_s||_row the caller has cached:
 * colscale_s [n_s] bf16, one for every present segment (2-byte aligned).  Per output feature: z = bf16(x . W^T + lora_scale * t . bext[row]),
 * v = bf16(z * colscale[row]) - the roundings of out * (m / norm) in the bf16 eager graph -, then the epilogue of llx_gemv_bf16 on v
 * (q and k are scaled before RoPE, gate and up each by their own factor before SwiGLU).  Every other operand as llx_gemv_bf16. */
int llx_gemv_bf16_dora(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2, int64_t n2,
                       const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out, int64_t ldo,
                       const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache, int64_t c_sh,
                       int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1, const void* bext2, int64_t rank0, int64_t rank1,
                       int64_t rank2, const void* t, int64_t ldt, float lora_scale, const void* colscale0, const void* colscale1,
                       const void* colscale2, llx_stream_t s);
/* ---- OCP MXFP4 weight-only linears (subclasses/mxfp4.py).  A weight [N, K], K % 32 == 0, is packed uint8 [N, K/2] (byte j =
 * element 2j in bits 0-3, element 2j+1 in bits 4-7; code = sign << 3 | e2m1, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6) and scale uint8
 * [N, K/32] (biased exponent b of a block of 32 consecutive k of a row; block scale 2^(b - 127)).
 * Quantise, in fp32: amax = max |x| of the block; b = 127 when amax == 0, else e = clamp(floor(log2 amax) - 2, -125, 125), b = e + 127;
 * |x| * 2^-e rounded to the nearest magnitude, ties to the code with mantissa bit 0, above 6 saturated; the sign bit is the input's.
 * x: bf16 (is_f32 = 0) or fp32 (1), row stride ldx elements (rows 16-byte aligned); packed and scale contiguous.  Non-finite input is
 * the caller's to refuse. */
int llx_quantize_mxfp4(const void* x, int64_t ldx, int is_f32, int64_t N, int64_t K, void* packed, void* scale, llx_stream_t s);
/* The bf16 image magnitude * 2^(b - 127) (exact; never a denormal for the scales the quantiser emits): out [N, K] (ldo % 8 == 0), or with
 * transpose out [K, N] (ldo >= N).  ldw / lds: row strides of packed (bytes, % 16) and scale (bytes). */
int llx_dequantize_mxfp4(const void* packed, int64_t ldw, const void* scale, int64_t lds, int64_t N, int64_t K, void* out, int64_t ldo,
                         int transpose, llx_stream_t s);
/* llx_gemv_bf16 on MXFP4 weights: W_s = packed rows (ldw_s in bytes, % 16), scale_s / lds_s = their scale bytes and row stride, for every
 * present segment; K % 32 == 0; M in 1..4 (3 and 4 rows: two passes over the weights).  Norm, segments, epilogues and LoRA operands as
 * llx_gemv_bf16, and its rounding points: out = epilogue(bf16(x . dq(W)^T + lora_scale * t . bext[row])), fp32 sums, the adapter joins
 * the base in fp32 - an MXFP4 linear behaves as a bf16 linear whose weight is the dequantised image. */
int llx_gemv_mxfp4(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2, int64_t n2,
                   const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out, int64_t ldo,
                   const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache, int64_t c_sh,
                   int64_t c_ss, const int64_t* input_pos, const void* bext0, const void* bext1, const void* bext2, int64_t rank0, int64_t rank1,
                   int64_t rank2, const void* t, int64_t ldt, float lora_scale, const void* scale0, int64_t lds0, const void* scale1,
                   int64_t lds1, const void* scale2, int64_t lds2, llx_stream_t s);
/* *extent (device int) = 1 + the largest key index any of the `rows` bool mask rows (row stride in bytes) allows; 0 if none: the
 * mask of the cached path is data (rows of a tril matrix gathered at input_pos, :194,:205), its extent sizes the decode key ranges. */
int llx_mask_extent(const void* mask, int64_t row_stride, int64_t rows, int64_t Skv, int* extent, llx_stream_t s);
/* KVCache.update (:83-90): cache[b, h, input_pos[l], :] = src[b, h, l, :] for k and v (sources share strides, caches share strides). */
int llx_kv_scatter(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb, int64_t c_sh,
                   int64_t c_ss, const int64_t* input_pos, int64_t B, int64_t KVH, int64_t L, int64_t Smax, int64_t head_dim, llx_stream_t s);
/* KVCache.update for a batch whose sequences sit at their own positions: cache[b, h, input_pos[b, l], :] = src[b, h, l, :]
 * (input_pos int64 [B, L], row stride p_sb elements).  The kernel of llx_kv_scatter with a position row per batch element. */
int llx_kv_scatter_rows(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb,
                        int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t p_sb, int64_t B, int64_t KVH, int64_t L, int64_t Smax,
                        int64_t head_dim, llx_stream_t s);
/* ---- FP8 KV cache: a cache is uint8 [B, KVH, Smax, 128] of OCP E4M3 codes (e4m3fn: bias 7, normals from 2^-6, subnormals
 * in steps of 2^-9, no infinities), no scale; every cache stride below is in BYTES.  q(x), on the bf16 value x the bf16 cache would have
 * held: clamp to [-448, 448], round to nearest even on the E4M3 grid, the sign bit is the input's (zero too), +-inf saturates, NaN stays
 * a NaN code.  dq(code) is exact in bf16.  An FP8 cache behaves as a bf16 cache that holds dq(q(x)) wherever the bf16 cache holds x.
 * The two scatters are llx_kv_scatter / llx_kv_scatter_rows with q() on the way (an out-of-range position writes nothing); sources
 * bf16 through element strides (% 8), cache strides % 16, all pointers 16-byte aligned. */
int llx_kv_scatter_f8(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb, int64_t c_sh,
                      int64_t c_ss, const int64_t* input_pos, int64_t B, int64_t KVH, int64_t L, int64_t Smax, int64_t head_dim, llx_stream_t s);
int llx_kv_scatter_rows_f8(const void* k, const void* v, int64_t s_sb, int64_t s_sh, int64_t s_ss, void* k_cache, void* v_cache, int64_t c_sb,
                           int64_t c_sh, int64_t c_ss, const int64_t* input_pos, int64_t p_sb, int64_t B, int64_t KVH, int64_t L, int64_t Smax,
                           int64_t head_dim, llx_stream_t s);
/* out bf16 [B, KVH, S, 128] contiguous = dq(cache [B, KVH, S, 128] through byte strides % 16): the transient image the prefill kernels read. */
int llx_kv_dequantize_f8(const void* cache, int64_t c_sb, int64_t c_sh, int64_t c_ss, void* out, int64_t B, int64_t KVH, int64_t S,
                         int64_t head_dim, llx_stream_t s);
/* The weight streams write an FP8 cache through epilogue 4: epilogue 2 (q|k|v) of every llx_gemv_* / llx_gemm_rows16_* entry point with
 * k_cache / v_cache pointing at codes and c_sb / c_sh / c_ss in bytes (% 4, pointers 4-byte aligned); the k / v branch stores q() of the
 * bf16 values epilogue 2 would have stored, the q rows are unchanged. */
/* The product of llx_gemv_bf16 for 2 <= M <= 16 activation rows (a batch of sequences, one token each) on the matrix pipe:
 * out = epilogue( [rmsnorm(x) | x][M, K] . [W0; W1; W2]^T ) with v_mfma_f32_16x16x32_bf16 (rows padded to 16 with zeros in registers),
 * fp32 accumulation, every weight element read from HBM once whatever M is.  bf16 weights without adapters; W_s [n_s, K] row-major
 * (inner n_s % 16 == 0), K % 8 == 0, K <= 32768.  K is split over workgroups where the tiles alone do not fill the machine; the
 * fp32 partial tiles go through the workspace (llx_gemm_rows16_workspace_bytes(M, N, K, epilogue) bytes, 16-byte aligned, not shared
 * with a call on another stream; 0 = no split) and a second small launch sums them in a fixed order and runs the epilogue:
 * deterministic, repeat calls are bit-identical.
 * Epilogues 0, 1, 3 as llx_gemv_bf16.  Epilogue 2 (q|k|v) is the BATCHED mode: row m is sequence m at token index 0 of the call, so
 * apply_rope uses table row 0 on the q and k heads; q -> out [M, n_q]; k / v heads -> cache[m] at pos[m] (device int64 [M]; a position
 * outside [0, Smax) writes nothing), caches [>= M, KVH, Smax, 128] through (batch, head, position) strides. */
int64_t llx_gemm_rows16_workspace_bytes(int64_t M, int64_t N, int64_t K, int epilogue);
int llx_gemm_rows16_bf16(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2, int64_t n2,
                         const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out, int64_t ldo,
                         const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache, int64_t c_sb,
                         int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos, void* workspace, int64_t workspace_bytes, llx_stream_t s);
/* llx_gemm_rows16_bf16 on int8 weight rows of the DYNAMIC kind (dynamic_int8_act, subclasses/int8.py:112-113; there is no flag: the
 * weight-only kind has no batched stream): W_s [n_s, K] int8 row-major (ldw_s in bytes, % 16), scale_s [n_s] bf16 per-row scales,
 * K % 16 == 0.  Each (normalised) row of x is quantised in the prologue as llx_quantize_int8_rowwise does (absmax of the whole row),
 * v_mfma_i32_16x16x64_i8 into int32, out = bf16(((float)acc * x_scale[m]) * scale[row]) - bit-exact with the reference
 * (int8_mm.py:93-118) and with llx_gemv_i8(dynamic = 1) when no norm is fused - then the epilogues of llx_gemm_rows16_bf16.  A split K
 * sums int32 partial tiles (exact in any order); the workspace (llx_gemm_rows16_i8_workspace_bytes() bytes, 16-byte aligned; 0 = no
 * split) holds a 16-float header of activation-row scales in front of them. */
int64_t llx_gemm_rows16_i8_workspace_bytes(int64_t M, int64_t N, int64_t K, int epilogue);
int llx_gemm_rows16_i8(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2, int64_t n2,
                       const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out, int64_t ldo,
                       const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache, int64_t c_sb,
                       int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos, void* workspace, int64_t workspace_bytes,
                       const void* scale0, const void* scale1, const void* scale2, llx_stream_t s);
/* The two products above on LoRA / DoRA linears (modelling/lora.py:43,51-59), the leading arguments unchanged.  bext_s: bf16
 * [n_s, rank_s] row-major, one for every present weight (and none for an absent one), 16-byte aligned; rank_s a multiple of 16, at most
 * 64; t: bf16 [M, sum rank] = [rmsnorm(x) | x] . [A_0; A_1; A_2]^T from a call of llx_gemm_rows16_bf16 on the A factors, 16-byte
 * aligned, ldt % 8 == 0.  The adapter term of a finished 16 x 16 tile is a short v_mfma_f32_16x16x32_bf16 chain where the tile's
 * epilogue runs (main launch, or the combine launch of a split K); workspaces as the un-adapted entry points.  Rounding points of
 * llx_gemv_bf16 / llx_gemv_bf16_dora / llx_gemv_i8(dynamic = 1):
 *   bf16 rows:  v = bf16(acc + lora_scale * t_s . bext_s[row]); colscale_s (bf16 [n_s], DoRA's cached row factors; for every present
 *               segment or for none): v = bf16(v * colscale_s[row]);
 *   int8 rows:  v = bf16(bf16(((float)acc * x_scale[m]) * scale[row]) + lora_scale * t_s . bext_s[row]);
 * then the epilogue.  Bad ranks, a weight without its factor (or the reverse), a null t and partial colscale are LLX_ERR_ARG. */
int llx_gemm_rows16_bf16_lora(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                              int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out,
                              int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache,
                              int64_t c_sb, int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos, void* workspace, int64_t workspace_bytes,
                              const void* bext0, const void* bext1, const void* bext2, int64_t rank0, int64_t rank1, int64_t rank2, const void* t,
                              int64_t ldt, float lora_scale, const void* colscale0, const void* colscale1, const void* colscale2, llx_stream_t s);
int llx_gemm_rows16_i8_lora(const void* w0, int64_t ldw0, int64_t n0, const void* w1, int64_t ldw1, int64_t n1, const void* w2, int64_t ldw2,
                            int64_t n2, const void* x, int64_t ldx, int64_t M, int64_t K, const void* norm_w, float eps, int epilogue, void* out,
                            int64_t ldo, const void* res, int64_t ldr, const float* rope, int64_t n_q, int64_t n_k, void* k_cache, void* v_cache,
                            int64_t c_sb, int64_t c_sh, int64_t c_ss, int64_t Smax, const int64_t* pos, void* workspace, int64_t workspace_bytes,
                            const void* scale0, const void* scale1, const void* scale2, const void* bext0, const void* bext1, const void* bext2,
                            int64_t rank0, int64_t rank1, int64_t rank2, const void* t, int64_t ldt, float lora_scale, llx_stream_t s);
/* SDPA(q, k_cache, v_cache, mask, is_causal=False, enable_gqa=True) (:135-137) for M query tokens with M * H / KVH <= 16: the cache of a
 * kv head is split over `nsplit` workgroups, the heads of its group share every K / V row read; partials merged in a second launch.
 * q / o [B, H, M, 128], caches [B, KVH, Skv, 128] through (batch, head, position) strides; mask bool [.., M, Skv] with broadcast
 * strides; extent nullable (llx_mask_extent); workspace fp32, llx_attn_decode_workspace_bytes(B, H, M, nsplit) bytes. */
int64_t llx_attn_decode_workspace_bytes(int64_t B, int64_t H, int64_t M, int64_t nsplit);
int llx_attn_decode(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k_cache, const void* v_cache, int64_t c_sb, int64_t c_sh,
                    int64_t c_ss, void* o, int64_t o_sb, int64_t o_sh, int64_t o_ss, const void* mask, int64_t m_sb, int64_t m_sh, int64_t m_sq,
                    const int* extent, float* workspace, int64_t B, int64_t H, int64_t KVH, int64_t M, int64_t Skv, int64_t nsplit,
                    int64_t head_dim, float scale, llx_stream_t s);
/* llx_attn_decode over FP8 caches: uint8 [B, KVH, Skv, 128] of E4M3 codes through byte strides (% 8, pointers 16-byte aligned), unpacked
 * with the hardware conversion; the same lane layout, split plan, mask handling, partials, combine launch and workspace, and the result
 * of llx_attn_decode on the caches' bf16 images. */
int llx_attn_decode_f8(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k_cache, const void* v_cache, int64_t c_sb, int64_t c_sh,
                       int64_t c_ss, void* o, int64_t o_sb, int64_t o_sh, int64_t o_ss, const void* mask, int64_t m_sb, int64_t m_sh, int64_t m_sq,
                       const int* extent, float* workspace, int64_t B, int64_t H, int64_t KVH, int64_t M, int64_t Skv, int64_t nsplit,
                       int64_t head_dim, float scale, llx_stream_t s);

/* ---- RoPE: apply_rope at modelling/llama.py:63-73 (in place on the first `nheads` 128-wide heads of each row;
 *      table fp32 [S,64,2] from build_rope :54-60); backward = rotation by -theta. ----------------------------- */
int llx_rope(const void* x, int64_t x_sb, int64_t x_ss, void* y, int64_t y_sb, int64_t y_ss, const float* table, int64_t B, int64_t S,
             int64_t nheads, int64_t head_dim, int backward, llx_stream_t s);

/* ---- SwiGLU: silu(w1 x) * w3 x at modelling/llama.py:152 --------------------------------------------------------- */
int llx_swiglu_fwd(const void* g, int64_t g_ld, const void* u, int64_t u_ld, void* h, int64_t h_ld, int64_t rows, int64_t cols, llx_stream_t s);
int llx_swiglu_bwd(const void* dh, int64_t dh_ld, const void* g, int64_t g_ld, const void* u, int64_t u_ld, void* dg, int64_t dg_ld,
                   void* du, int64_t du_ld, int64_t rows, int64_t cols, llx_stream_t s);

/* ---- embedding: nn.Embedding at modelling/llama.py:180,206 / modelling/audio.py:49; strided destination lets the
 *      gather land behind the audio prefix (replaces torch.cat at modelling/audio.py:63). ------------------------- */
int llx_embedding_fwd(const int64_t* ids, const void* table, void* out, int64_t n_tok, int64_t dim, int64_t vocab, int64_t tok_per_batch,
                      int64_t out_sb, int64_t out_ss, llx_stream_t s);
int llx_embedding_bwd(const int64_t* ids, const void* dy, float* dtable_f32, int64_t n_tok, int64_t dim, int64_t vocab,
                      int64_t tok_per_batch, int64_t dy_sb, int64_t dy_ss, llx_stream_t s);

/* ---- fused cross-entropy: F.cross_entropy(logits.float(), labels) at modelling/llama.py:218, modelling/audio.py:76
 *      (ignore_index -100, mean).  dlogits may alias logits (nullable = forward only). --------------------------- */
int64_t llx_ce_workspace_bytes(int64_t T);
int llx_ce_fwd_bwd(const void* logits, int64_t ld, void* dlogits, int64_t dld, const int64_t* labels, float* loss, void* workspace,
                   int64_t T, int64_t V, llx_stream_t s);
/* ---- LM-head row compaction.  F.cross_entropy(ignore_index=-100) (modelling/llama.py:216-218, modelling/audio.py:74-76): a position
 *      whose label is -100 adds nothing to the loss and has a zero gradient row, so norm -> head -> CE -> d hidden only need the
 *      labelled rows.  They are compacted IN ORDER on the device; the count never visits the host (hipGraph-capturable):
 *        llx_head_compact_index: idx[j] = position of the j-th labelled row (-1 for j >= count), inv[i] = j or -1,
 *                                labels_c[j] = labels[idx[j]] (-100 beyond), count[0] = number of labelled rows
 *        llx_gather_rows:        dst[j] = src[idx[j]] (j < count); zero rows up to the next multiple of 256; later rows untouched
 *        llx_gemm_nt_bf16_rows / llx_ce_fwd_bwd_rows: the head GEMMs / the loss over the compacted rows (rows = count)
 *        llx_scatter_rows:       dst[i] = bf16(scale[0] * src[inv[i]]) where inv[i] >= 0, zero rows elsewhere
 *      Loss and every gradient equal the uncompacted computation (same per-row arithmetic; the loss sums the same row terms). */
int llx_head_compact_index(const int64_t* labels, int32_t* idx, int32_t* inv, int64_t* labels_c, int32_t* count, int64_t T, llx_stream_t s);
int llx_gather_rows(const void* src, int64_t ld_src, const int32_t* idx, const int32_t* count, void* dst, int64_t ld_dst, int64_t T, int64_t D,
                    llx_stream_t s);
int llx_scatter_rows(const void* src, int64_t ld_src, const int32_t* inv, const float* scale /* nullable */, void* dst, int64_t ld_dst,
                     int64_t T, int64_t D, llx_stream_t s);
int llx_ce_fwd_bwd_rows(const void* logits, int64_t ld, void* dlogits, int64_t dld, const int64_t* labels, float* loss, void* workspace,
                        int64_t T, int64_t V, const int32_t* rows, llx_stream_t s);
/* the same loss over a row set walked in chunks (one logits buffer per chunk; labels / workspace cover all T rows): phase bit 0 = first
 * chunk (count the labelled rows of the whole set), bit 1 = last chunk (reduce into loss); values identical to one call over all rows */
int llx_ce_fwd_bwd_part(const void* logits, int64_t ld, void* dlogits, int64_t dld, const int64_t* labels, float* loss, void* workspace, int64_t T,
                        int64_t V, int64_t row0, int64_t nrows, const int32_t* rows, int phase, llx_stream_t s);

/* ---- per-token log-probabilities: -F.cross_entropy(logits.float(), labels, reduction="none", ignore_index=-100), the per-row terms of
 *      the mean above, with a per-row upstream gradient.  fwd: logp[t] = x[label] - lse[t] (0 / 0 on ignored rows), top1 (nullable) =
 *      argmax of the row, lowest index among ties, -1 on ignored rows; one read of the row, the logits are kept.  bwd:
 *      dlogits[t, v] = bf16(g[t] * ((v == label) - exp(x[t, v] - lse[t]))), one rounding; zero rows where ignored or g[t] == 0;
 *      dlogits may alias logits.  rows (nullable): as llx_ce_fwd_bwd_rows - rows at or past *rows rounded up to 256 are not read;
 *      fwd writes zeros there, bwd nothing. ------------------------------------------------------------------------------ */
int llx_logprob_rows_fwd(const void* logits, int64_t ld, const int64_t* labels, float* logp, float* lse, int32_t* top1 /* nullable */,
                         int64_t T, int64_t V, const int32_t* rows /* nullable */, llx_stream_t s);
int llx_logprob_rows_bwd(const void* logits, int64_t ld, void* dlogits, int64_t dld, const int64_t* labels, const float* lse, const float* g,
                         int64_t T, int64_t V, const int32_t* rows /* nullable */, llx_stream_t s);
/* the [T] vectors between positions and compacted rows (logp / top1 through inv, the upstream gradient through idx), one launch:
 * dst[i] = map[i] >= 0 ? src[map[i]] : fill, for a float vector and (nullable pair) an int32 vector */
int llx_logprob_map_rows(const int32_t* map, const float* src_f, float* dst_f, float fill_f, const int32_t* src_i /* nullable */,
                         int32_t* dst_i /* nullable */, int32_t fill_i, int64_t T, llx_stream_t s);

/* ---- the k likeliest tokens of a row as log-probabilities (csrc/topk.hip), 1 <= k <= 8, bf16 logits [R, V] with row stride ld,
 *      V % 8 == 0: ids[r, j] (int32) / logp[r, j] (fp32), j < k, descending by value, equal values by ascending index (the tie rule of
 *      top1 and of the greedy sampler; -0.0 == +0.0; -inf last, by index; a NaN ranks as -inf), so ids[r, 0] is the top1 of
 *      llx_logprob_rows_fwd.  logp = x - lse[r] with lse given (fp32 [R]); with lse null the kernel forms it as llx_logprob_rows_fwd
 *      does, logp = (x - max) - log(sum).  label_logp (nullable; with labels and lse): the alternative that is the row's label gets
 *      label_logp[r].  One read of the row for the selection; no atomics: repeat launches are bit-identical.
 *      scoring (labels given): row r writes at ids / logp + r * ld_out; rows with label -100 and rows at or past *rows (nullable)
 *        rounded up to 256 are not read and get ids = -1, logp = 0.
 *      generation (pos given; finished nullable; the geometry of the sampler's history): row r writes [k] values at
 *        r * ld_out + (pos[r] - hist_base) * k when that column lies in [0, hist_cap) and finished[r] is not set, else nothing;
 *        pos and finished are only read - launched before the sampler of the step it sees the column the sampler then fills.
 *      neither: every row is ranked and written at r * ld_out. -------------------------------------------------------------------- */
int llx_topk_logprobs_rows(const void* logits, int64_t ld, int64_t R, int64_t V, int k, const float* lse /* nullable */,
                           const float* label_logp /* nullable */, const int64_t* labels /* nullable */, const int32_t* rows /* nullable */,
                           const int64_t* pos /* nullable */, int64_t hist_base, const int32_t* finished /* nullable */, int32_t* ids,
                           float* logp, int64_t ld_out, int64_t hist_cap, llx_stream_t s);
/* the [T, k] results of the compacted rows back to their positions: dst[i, :] = map[i] >= 0 ? src[map[i], :] : (-1, 0.0) */
int llx_topk_map_rows(const int32_t* map, const int32_t* src_ids, const float* src_logp, int32_t* dst_ids, float* dst_logp, int64_t T, int k,
                      llx_stream_t s);

/* ---- LoRA skinny contractions (modelling/lora.py:43 and its autograd): T = X.W^T -> [M,64] zero padded;
 *      G = s * U^T.Y with fp32 split partials (deterministic). --------------------------------------------------- */
int llx_skinny_nt(const void* X, int64_t ldx, const void* W, int64_t ldw, void* out, int64_t M, int64_t K, int64_t R,
                  const int32_t* kranges /* host, nullable: {lo,hi} x 4 per 16 rows of a block-diagonal W */, llx_stream_t s);
/* llx_skinny_nt that also writes G[M,K] = bf16(X * colscale[k]) (row stride ldg) from the same read of X: the (grad_output * scale)
 * operand of a weight-only int8 linear's data gradient (subclasses/int8.py:127) rides in the adapter's dy @ lora_b pass. */
int llx_skinny_nt_scaled(const void* X, int64_t ldx, const void* W, int64_t ldw, void* out, int64_t M, int64_t K, int64_t R,
                         const int32_t* kranges, const void* colscale, void* G, int64_t ldg, llx_stream_t s);
/* nn.RMSNorm (modelling/llama.py:158-160) and the adapter's x @ lora_a^T on its output (modelling/lora.py:43) from ONE read of x:
 * y = rmsnorm(x) [M,D], rstd fp32 [M], t = y . W^T [M,64 padded] (W = the group's stacked lora_a [R,D]).  D % 512 == 0, D <= 4096. */
int llx_rmsnorm_skinny_nt(const void* x, const void* g, const void* W, int64_t ldw, void* y, float* rstd, void* t, int64_t M, int64_t D,
                          int64_t R, float eps, llx_stream_t s);
int64_t llx_skinny_tn_workspace_bytes(int64_t M, int64_t N, int64_t R);
int llx_skinny_tn(const void* U, const void* Y, int64_t ldy, void* out, int64_t out_ld, int64_t M, int64_t N, int64_t R, float scale,
                  int transpose_out, int accumulate, void* workspace,
                  const int32_t* segs /* host, nullable: {n_lo, n_hi, r_lo, r_hi} per member of a fused group; member blocks are
                                         then written one after another as contiguous [n, r] matrices */, int seg_count, llx_stream_t s);
/* the two stages of llx_skinny_tn separately: the fp32 split partials of one product, and the second stage of up to 4 products (the
 * adapter gradients of one transformer block) in ONE launch; host arrays of length n, entry i = the arguments of product i */
int llx_skinny_tn_partial(const void* U, const void* Y, int64_t ldy, int64_t M, int64_t N, int64_t R, void* workspace, const int32_t* segs,
                          int seg_count, llx_stream_t s);
/* first stage of up to 4 products in ONE launch (the d lora_b and d lora_a products of a linear group: different operands, ready together) */
int llx_skinny_tn_partial_many(int n, const void* const* U, const void* const* Y, const int64_t* ldy, const int64_t* M, const int64_t* N,
                               const int64_t* R, void* const* workspaces, const int32_t* const* segs, const int* seg_count, llx_stream_t s);
/* ... where product i with upart[i] != NULL also emits, from the Y tiles it stages anyway, the column-tile partial sums of  u = Y_i . Bt_i^T
 * (the adapter's dy @ B of modelling/lora.py:43's backward; Bt_i [R_i, N_i] bf16 row-major with row stride ldb[i], the batched
 * block-diagonal B^T of a fused group; upart[i]: llx_skinny_u_workspace_bytes(M_i, N_i) bytes): dy is read once for dB and u.
 * llx_skinny_u_reduce sums the tiles into u [M, 64] bf16 (columns >= R zero); segs / seg_count as given to the product. */
int64_t llx_skinny_u_workspace_bytes(int64_t M, int64_t N);
int llx_skinny_tn_partial_many_u(int n, const void* const* U, const void* const* Y, const int64_t* ldy, const int64_t* M, const int64_t* N,
                                 const int64_t* R, void* const* workspaces, const int32_t* const* segs, const int* seg_count,
                                 const void* const* Bt, const int64_t* ldb, void* const* upart, llx_stream_t s);
int llx_skinny_u_reduce(const void* upart, void* out, int64_t M, int64_t N, int64_t R, const int32_t* segs, int seg_count, llx_stream_t s);
/* ... and product i with G[i] != NULL also writes G_i[m, n] = bf16(Y_i[m, n] * colscale_i[n]) (row stride ldg[i]): the (grad_output * scale)
 * operand of an int8 linear's data gradient (subclasses/int8.py:127) from the same read of dy. */
int llx_skinny_tn_partial_many_us(int n, const void* const* U, const void* const* Y, const int64_t* ldy, const int64_t* M, const int64_t* N,
                                  const int64_t* R, void* const* workspaces, const int32_t* const* segs, const int* seg_count,
                                  const void* const* Bt, const int64_t* ldb, void* const* upart, const void* const* colscale,
                                  void* const* G, const int64_t* ldg, llx_stream_t s);
int llx_skinny_tn_reduce_many(int n, const void* const* workspaces, void* const* outs, const int64_t* out_ld, const int64_t* M, const int64_t* N,
                              const int64_t* R, const float* scale, const int* transpose_out, const int* accumulate,
                              const int32_t* const* segs, const int* seg_count, llx_stream_t s);
int llx_pad64(const void* in, int64_t ld, void* out, int64_t R, int64_t C, float scale, int transpose, llx_stream_t s);
int llx_lora_group_pack(const void* const* lora_a, const void* const* lora_b, const int64_t* Ns, const int64_t* ranks, int nm, int64_t K,
                        float scale, void* a_cat, void* b2, void* bT, void* a2t, llx_stream_t s);  /* all four images, one launch (host arrays) */
int llx_lora_groups_pack(const void* const* lora_a, const void* const* lora_b, const int64_t* Ns, const int64_t* ranks, const int* nm,
                         const int64_t* K, const float* scale, void* const* a_cat, void* const* b2, void* const* bT, void* const* a2t, int ng,
                         llx_stream_t s);  /* the same for up to 4 groups (one transformer layer) in one launch; host arrays, group j's members at 4*j+i */
int llx_lora_pack(const void* in, int64_t ld, void* out, int64_t out_ld, int64_t R, int64_t C, int64_t row_off, int64_t col_off, float scale,
                  int transpose, llx_stream_t s);   /* batched LoRA operand images of a linear group (q|k|v, gate|up) */

/* ---- DoRA (modelling/lora.py:47-62): out = (x W^T + s x A^T B^T) * m / ||W + s B A||_row (+ bias).  The row norm is evaluated from
 *      ||W_n||^2 (llx_rownorm2, cached per frozen weight), G = W A^T and A A^T (llx_skinny_nt) - no dense [out,in] temporary;
 *      llx_dora_colscale -> c = m / norm (bf16, the column scale: llx_scale / llx_colscale_bias / GEMM epilogue 4) and 1/norm (fp32);
 *      llx_colsum_mul -> d m[n] = (sum_rows dy * z)[n] / norm[n], two deterministic stages. --------------------------------- */
int llx_rownorm2(const void* W, int64_t ld, float* out, int64_t rows, int64_t cols, llx_stream_t s);
int llx_dora_colscale(const float* wn2, const void* G /*bf16 [N,64]*/, const void* b2 /*bf16 [N,64] = s*B*/, const void* AAt /*bf16 [R,64]*/,
                      const void* m /*bf16 [N]*/, void* c /*bf16 [N]*/, float* inv_norm /*fp32 [N]*/, int64_t N, int64_t R, llx_stream_t s);
int64_t llx_colsum_mul_workspace_bytes(int64_t N);
int llx_colsum_mul(const void* a, int64_t lda, const void* b, int64_t ldb, const float* colscale /*nullable fp32 [N]*/, void* out /*bf16 [N]*/,
                   void* workspace, int64_t M, int64_t N, llx_stream_t s);
int llx_colscale_bias(const void* x, int64_t x_ld, void* y, int64_t y_ld, const void* colscale /*bf16 [cols]*/, const void* bias /*nullable*/,
                      int64_t rows, int64_t cols, llx_stream_t s);

/* ---- audio front end (modelling/audio.py:26-36,53-60): MelSpectrogram(n_fft 512, win 400, hop 160, 128 slaney mels,
 *      power 2, centre/reflect) -> log10/clip/CMN -> bf16 time-major padded features; exact-erf GELU; conv k=3 helpers.
 *      twiddle fp32 [512][2], window fp32 [512], fbank fp32 [257][n_mels] are host-built constants. --------------- */
int llx_mel_spectrogram(const float* audio, int64_t B, int64_t L, const float* twiddle, const float* window, const float* fbank, float* mel,
                        int64_t n_frames, int64_t hop, int64_t n_mels, llx_stream_t s);
int llx_logmel_cmn(const float* mel, void* feat /* bf16 [B, n_frames+1, n_mels] */, int64_t B, int64_t n_frames, int64_t n_mels, llx_stream_t s);
int llx_gelu_fwd(const void* z, int64_t z_ld, void* y, int64_t y_ld, int64_t rows, int64_t cols, llx_stream_t s);
int llx_gelu_bwd(const void* dy, int64_t dy_ld, const void* z, int64_t z_ld, void* dz, int64_t dz_ld, int64_t rows, int64_t cols, llx_stream_t s);
int llx_col2im3(const void* dA, void* dpad, int64_t M, int64_t C, int64_t P, int64_t stride, llx_stream_t s);
int llx_conv_w_reorder(const void* in, void* out, int64_t D, int64_t C, int to_gemm, llx_stream_t s);

/* ---- token sampler (llx/generate.py; the reference has no generate(): this is the loop behind its `input_pos` branch,
 *      modelling/llama.py:204-205).  One token for each of R rows of logits [R, V] (dtype 0 = bf16, 1 = fp32; row stride ld >= V elements,
 *      rows may start at any element): temperature 0 = argmax (lowest index among ties); otherwise z = logit / temperature, top_k
 *      (0 = off; ties at the k-th value all stay), top_p (1 = off; keep i iff the weight of z_j > z_i is < top_p * W), then the first
 *      kept index whose running weight exceeds u * W, u = float(mix(mix(mix(seed) ^ pos[r]) ^ r) >> 40) * 2^-24 (splitmix64 finaliser).
 *      pos: DEVICE int64 [R], the draw counter (read on the device; advance != 0 stores pos + 1 back after the read).  token_out: int64
 *      [R].  history (nullable): int64 [R, cap], row stride hist_ld; the token goes to history[r, pos[r] - hist_base] when inside
 *      [0, cap).  finished (nullable, int32 [R]): a row whose flag is set writes eos_id and nothing else; a row that samples eos_id
 *      sets it.  aux_u / aux_thresh (fp32 [R]) / aux_kept (int32 [R]), nullable: the uniform, the raw logit of the smallest kept
 *      token, the number of kept tokens (greedy: the maximum and the size of its tie group). --------------------------------- */
int llx_sample_rows(const void* logits, int dtype, int64_t ld, int64_t R, int64_t V, float temperature, int64_t top_k, float top_p,
                    uint64_t seed, int64_t* pos, int64_t* token_out, int64_t* history, int64_t hist_ld, int64_t hist_cap, int64_t hist_base,
                    int advance, int64_t eos_id, int32_t* finished, float* aux_u, float* aux_thresh, int32_t* aux_kept, llx_stream_t s);

/* ---- llx_sample_rows with sampler penalties and the token's log-probability (llx/sampling.py rule 0); the arguments of
 *      llx_sample_rows keep their meaning.  counts (nullable): DEVICE int32 [R, ldc], ldc >= V, counts[r][i] = how often token i has
 *      occurred in row r's sequence.  Null: no penalties, whatever the three floats are.  Otherwise every element with a count c > 0 is
 *      read as x = x > 0 ? x / repetition_penalty : x * repetition_penalty, then x - (presence_penalty + frequency_penalty * c), single
 *      fp32 operations in that order; argmax, temperature, top_k, top_p, the draw and aux_thresh all see the penalised value; after the
 *      draw counts[r][token] += 1 (a finished row touches neither counts nor logprob_history).  repetition_penalty finite and > 0 (1 =
 *      off), the other two finite (0 = off).  logprob_history (nullable; needs history, whose row stride, cap and base it shares): fp32,
 *      receives (l_tok - l_max) - log sum exp(l - l_max) over the RAW logits - no penalty, temperature 1, nothing filtered - at
 *      [r, pos[r] - hist_base] when inside [0, cap). ---------------------------------------------------------------------------- */
int llx_sample_rows_ext(const void* logits, int dtype, int64_t ld, int64_t R, int64_t V, float temperature, int64_t top_k, float top_p,
                        uint64_t seed, int64_t* pos, int64_t* token_out, int64_t* history, int64_t hist_ld, int64_t hist_cap, int64_t hist_base,
                        int advance, int64_t eos_id, int32_t* finished, float* aux_u, float* aux_thresh, int32_t* aux_kept, int32_t* counts,
                        int64_t ldc, float repetition_penalty, float presence_penalty, float frequency_penalty, float* logprob_history,
                        llx_stream_t s);

/* ---- prompt-lookup drafting (generate(draft_tokens=k), llx/generate.py): the bookkeeping of one greedy speculative step, one workgroup,
 *      no host read.  The step fed step_tok [k + 1] = [last token, k draft tokens] at step_pos; picks int64 [k + 1] are the greedy picks of
 *      its k + 1 logits rows.  With a = the longest prefix with step_tok[1 + i] == picks[i], picks[0 .. a] are emitted - cut to the room
 *      left (P + n - len[0]) and after the first eos_id (-1: none; it sets finished[0]) - and appended to seq (int64 [cap], cap >= P + n:
 *      the prompt, then the generated tokens; len int64 [1]).  Then the next step is written: step_tok = [seq[len - 1], draft],
 *      step_pos = len - 1 .. len - 1 + k, the draft by llx.sampling.lookup_draft (the most recent earlier occurrence of the last gg
 *      tokens, gg = g .. 1, the longest first, continued; no match repeats the last token).  counters int64 [2] += (1, emitted - 1).
 *      init != 0: the first token after the prefill - picks [1] is emitted, nothing is confirmed, step_tok is not read.  A launch that
 *      finds finished[0] set or len[0] == P + n changes nothing.  k in 1..3, g in 1..8, P >= 1, n >= 1.  The caller keeps
 *      len - 1 + k inside the KV cache. ---------------------------------------------------------------------------------------- */
int llx_lookup_step(const int64_t* picks, int64_t* seq, int64_t cap, int64_t* len, int64_t* step_tok, int64_t* step_pos, int32_t* finished,
                    int64_t* counters, int64_t P, int64_t n, int k, int g, int64_t eos_id, int init, llx_stream_t s);

/* ---- beam search (generate(num_beams=W), llx/generate.py; the rule is llx.sampling.beam_shortlist / beam_step).  Three
 *      launches per step, no host read.
 *      llx_beam_rows: logits [W, V] (dtype 0 = bf16, 1 = fp32; row stride ld >= V elements, rows may start at any element; V > W) ->
 *      cand_score fp32 / cand_token int32 [W, W + 1]: log-probability (z - zmax) - log sum exp(z - zmax) and index of each row's W + 1
 *      best tokens by (logit descending, index ascending).  The sum is over floor(expf(z - zmax) * 2^40) in uint64.
 *      llx_beam_merge: orders the W * (W + 1) candidates by (s[r] + cand_score descending, row, rank) and walks them: a token eos_id
 *      (-1: none) is a finished hypothesis of final score score / len^length_penalty (len = tokens generated, the eos counted) that
 *      enters the bank if there is room or it beats the worst entry; any other becomes live beam j: parent[j] = r (int32 [W]), tok[j]
 *      (int64 [W], the next step's input), s[j] (fp32 [W]); the walk stops at W live beams.  hist int64 [W, n] (row stride hist_ld) is
 *      permuted by parent and appended to; bank_tok int64 [W, n] (row stride bank_ld), bank_len int32 [W], bank_score fp32 [W];
 *      meta int32 [3] = (hypotheses in the bank, done, tokens generated).  done is set when the bank holds W or n tokens are generated;
 *      the live beams are then offered to the bank with s / len^length_penalty.  init != 0: the first step after the prefill - the
 *      state is not read and only row 0 takes part.  A launch that finds done set writes parent = identity and nothing else.
 *      llx_kv_reorder_rows: table = DEVICE array of n_caches base pointers of bf16 caches [>= W, KVH, Smax, 128] with the common
 *      element strides sb, sh, ss (multiples of 8; last dim dense), parent = DEVICE int32 [W] (a value outside [0, W) reads as "stays"):
 *      cache[b, :, :len] <- cache[parent[b], :, :len], b < W, in place in every cache.  Slots with parent[b] == b, positions >= len
 *      and slots >= W are not written.  W in 2..16, len in [1, Smax], head_dim 128. ------------------------------------------------ */
int llx_beam_rows(const void* logits, int dtype, int64_t ld, int64_t W, int64_t V, float* cand_score, int32_t* cand_token, llx_stream_t s);
int llx_beam_merge(const float* cand_score, const int32_t* cand_token, float* s, int32_t* parent, int64_t* tok, int64_t* hist, int64_t hist_ld,
                   int64_t* bank_tok, int64_t bank_ld, int32_t* bank_len, float* bank_score, int32_t* meta, int64_t W, int64_t n,
                   int64_t eos_id, float length_penalty, int init, llx_stream_t stream);
int llx_kv_reorder_rows(const void* const* table, int64_t n_caches, int64_t sb, int64_t sh, int64_t ss, const int32_t* parent, int64_t W,
                        int64_t KVH, int64_t len, int64_t Smax, int64_t head_dim, llx_stream_t s);

/* ---- small utilities of the backward pass ---------------------------------------------------------------------- */
int llx_scale(const void* x, int64_t x_ld, void* y, int64_t y_ld, const float* dev_scalar, float host_scale, const void* colscale,
              int64_t rows, int64_t cols, llx_stream_t s);   /* (g * scale) of subclasses/int8.py:127; loss-scale of dX */
int llx_add(const void* x, const void* y, void* z, int64_t n, llx_stream_t s);   /* residual joins (modelling/llama.py:172-173) */
int llx_transpose(const void* in, int64_t in_ld, void* out, int64_t out_ld, int64_t R, int64_t C, int src_is_i8, llx_stream_t s);
int llx_i8_to_bf16(const void* in, void* out, int64_t n, llx_stream_t s);         /* int_data.T.to(dtype) of subclasses/int8.py:118 */

#ifdef __cplusplus
}
#endif
#endif /* LLX_H */
