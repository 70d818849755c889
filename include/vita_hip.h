/*
 * vita_hip.h — C ABI of libvita_hip.so, the MI355X (gfx950) hot path of Long-VITA prefill.
 *
 * The reference (VITA-MLLM/Long-VITA) contains no native code: every kernel on this path is
 * reached from Python through a third-party package (flash_attn, transformer_engine, apex,
 * cuBLAS via torch.matmul).  Each entry point below therefore cites the *Python call site* of
 * the reference that it replaces (R/ = /root/reference, M/ = R/long_vita_megatron,
 * H/ = R/long_vita).  A reference-side binding is a ctypes stub.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless noted;
 *   - activations / weights are bf16 (uint16 bit pattern), indices int64, statistics fp32;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); nothing is
 *     allocated, retained or freed by the library;
 *   - return value: VITA_OK (0) or a negative VITA_ERR_* code; no C++ exception crosses the ABI.
 */
#ifndef VITA_HIP_H
#define VITA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VITA_OK 0
#define VITA_ERR_INVALID_ARG (-1)   /* null pointer, non-positive size, bad enum                */
#define VITA_ERR_UNSUPPORTED (-2)   /* shape outside what the gfx950 kernels are built for      */
#define VITA_ERR_LAUNCH (-3)        /* hipGetLastError() != hipSuccess after the launch          */

/* ABI version; bump on any signature change. */
int vita_abi_version(void);
/* Human-readable text for a VITA_ERR_* code (static storage). */
const char* vita_error_string(int code);

/* ---------------------------------------------------------------------------------------------
 * RMSNorm forward.   y = (x.float() * rsqrt(mean(x^2) + eps)).to(bf16) * w        [rows, cols]
 * Replaces M/core/transformer/custom_layers/transformer_engine.py:74-79 (RMSNorm._norm/forward;
 * the TE-fused equivalent on GPU, M/core/models/gpt/gpt_layer_specs.py:39).
 * rstd_out (fp32 [rows]) may be NULL; when given it holds rsqrt(mean(x^2)+eps) per row.
 * ------------------------------------------------------------------------------------------- */
int vita_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd_out,
                     int64_t rows, int cols, float eps, void* stream);

/* LayerNorm forward (biased variance, fp32 statistics), bf16 in/out.
 * Replaces torch.nn.LayerNorm at M/core/models/vision/vit_layer_specs.py (ViT block norms,
 * eps 1e-6) and M/pretrain_long_vita.py:443-446 (projector pre-norm, eps 1e-5). */
int vita_layernorm_fwd(const void* x, const void* w, const void* b, void* y,
                       int64_t rows, int cols, float eps, void* stream);

/* Logit post-processing, in place on the bf16 logits [rows, cols] of the selected rows (row stride ld elements):
 *   logits *= multiplier_scale (skipped when 0);  logits = tanh(logits / softcapping) * softcapping (skipped when 0)
 * with the reference's bf16 rounding after every step.  Replaces M/core/models/multimodal/gpt_vl_model.py:349-355
 * (args.output_multiplier_scale, args.output_logit_softcapping).  _bwd: grad *= scale * (1 - (y / cap)^2) from the
 * stored output y (autograd of the same expressions). */
int vita_logit_postprocess(void* logits, int64_t ld, int64_t rows, int64_t cols, float multiplier_scale,
                           float softcapping, void* stream);
int vita_logit_postprocess_bwd(const void* y, int64_t ldy, void* grad, int64_t ldg, int64_t rows, int64_t cols,
                               float multiplier_scale, float softcapping, void* stream);

/* Token choice on the device: repetition penalty, then greedy arg-max or temperature / top-k / top-p sampling, in the order
 * transformers' `generate` applies its processors for the checkpoint's generation config
 * (H/models/long_vita_qwen2_intern/generation_config.json:4-12: repetition_penalty 1.05, temperature 0.7, top_k 20, top_p 0.8;
 * tools/inference_long_vita.py:820-826,868 loads it, turns do_sample off and calls model.generate).  fp32 on the bf16 logits:
 *   x = float(logit);  seen[id] && penalty != 1:  x = x < 0 ? x * penalty : x / penalty
 *   !do_sample: token = arg-max x (equal maxima: the lowest id), kept = 1; temperature / top_k / top_p are ignored
 *   do_sample:  x /= temperature;  0 < top_k < cols keeps x >= (k-th largest x), every tie with it included;  0 < top_p < 1 keeps, of
 *     what is left, a token iff the softmax mass of all tokens with a STRICTLY higher score is < top_p (equal scores stay or go
 *     together; at least one token stays);  token = the first kept token, in ascending id, whose inclusive mass prefix exceeds
 *     u * (kept mass);  kept = the number of kept tokens.  Masses are exp(x - max) as 2^-40 fixed point: sums are exact, the result
 *     is bit-reproducible.
 *   mark_chosen && seen: seen[token] = 1 after the choice.
 * One row of `seen` is `cols` bytes; the workspace (16-byte aligned) holds the fp32 scores.  cols, ld % 8 == 0; logits 16-byte aligned;
 * cols <= 2^23 (the 64-bit mass sums cannot overflow), else VITA_ERR_UNSUPPORTED.
 * vita_token_seen_mark: seen[ids[i]] = 1; an id outside [0, vocab) sets *err_flag (may be NULL) and writes nothing. */
int vita_token_seen_mark(const int64_t* ids, int64_t n, uint8_t* seen, int64_t vocab, int32_t* err_flag, void* stream);
/* H/models/long_vita_qwen2_intern/generation_config.json:4-12; tools/inference_long_vita.py:820-826,868 */
int64_t vita_select_token_workspace_bytes(int64_t rows, int64_t cols);
/* H/models/long_vita_qwen2_intern/generation_config.json:4-12; tools/inference_long_vita.py:820-826,868 */
int vita_select_token(const void* logits /* bf16 [rows, ld] */, int64_t ld, int64_t rows, int64_t cols,
                      uint8_t* seen /* [rows, cols] bytes, may be NULL */, float repetition_penalty,
                      int do_sample, float temperature, int top_k, float top_p,
                      const float* u /* [rows] uniforms in [0,1), device; NULL iff !do_sample */,
                      int64_t* token_out /* [rows] */, int32_t* kept_out /* [rows], may be NULL */,
                      int mark_chosen, void* workspace, int64_t workspace_bytes, void* stream);

/* Prompt-lookup speculative decoding (transformers' generate(prompt_lookup_num_tokens=k) at the same call site).  Additions at ABI 19.
 * Neither entry synchronises with the host.
 * vita_ngram_draft: the candidate rule of PromptLookupCandidateGenerator.get_candidates on the device history hist[0, n),
 * n = clamp(*n_hist, 0, hist_cap):  for g = min(max_ngram, n - 1) down to 1 take the LEFTMOST i in [0, n - g] with
 * hist[i : i + g] == hist[n - g : n] and i + g < min(n, max_total); the candidate is hist[i + g : min(i + g + num_draft, n, max_total)],
 * cut in front of its first eos id.  The first g that has such an i ends the search, even when the cut leaves nothing.  No such i, or
 * max_total == n + 1: zero drafts.  draft_out [num_draft] (unused slots -1), n_draft_out [1].  One pass over the history for all g; an
 * order-independent 64-bit minimum in two stages through `workspace` (8-byte aligned, vita_ngram_draft_workspace_bytes, never
 * initialised by the caller): the result is deterministic.  An entry of hist never forms an address.  Null pointers, num_draft < 1,
 * max_ngram < 1: VITA_ERR_INVALID_ARG; num_draft > 7, n_eos > 8, max_ngram > 2^20, hist_cap >= 2^31: VITA_ERR_UNSUPPORTED.
 * vita_draft_verify: the greedy acceptance of one verify pass of t = 2 .. 8 rows.  a_i = the choice vita_select_token makes with
 * do_sample = 0 on row i when the penalised ids are seen U {draft[0 .. i - 1]} (a draft id outside [0, cols) penalises nothing, never
 * indexes seen and never equals an a_i); n_acc = the leading i < t - 1 with draft[i] == a_i; emitted = a_0 .. a_{n_acc}, cut BEHIND the
 * first one that is an eos id (stop = 1).  Then hist[n .. n + n_emit) = emitted while they fit hist_cap, *n_hist = min(n + n_emit,
 * hist_cap), seen[token] = 1 for each emitted token, record [t + 2] = {n_emit, stop, emitted[0 .. t - 1]} with unused slots -1.
 * A row in which no score exceeds -inf (all -inf or NaN) chooses id 0: the history and the byte map only ever see ids in [0, cols).
 * cols / ld / alignment as vita_select_token; t outside 2 .. 8: VITA_ERR_UNSUPPORTED. */
/* tools/inference_long_vita.py:820-826,868 */
int64_t vita_ngram_draft_workspace_bytes(int64_t hist_cap);
/* tools/inference_long_vita.py:820-826,868 */
int vita_ngram_draft(const int64_t* hist, int64_t hist_cap, const int32_t* n_hist, int max_ngram, int num_draft,
                     int64_t max_total, const int64_t* eos, int n_eos, int64_t* draft_out, int32_t* n_draft_out,
                     void* workspace, int64_t workspace_bytes, void* stream);
/* tools/inference_long_vita.py:820-826,868 */
int vita_draft_verify(const void* logits, int64_t ld, int t, int64_t cols, uint8_t* seen, float repetition_penalty,
                      const int64_t* draft, const int64_t* eos, int n_eos, int64_t* hist, int64_t hist_cap, int32_t* n_hist,
                      int64_t* record, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RoPE.  Replaces M/core/models/common/embeddings/rotary_pos_embedding.py:84-122 (table),
 * :181-204 (apply_rotary_pos_emb_bshd) and apex fused_apply_rotary_pos_emb (:248-252).
 *
 * vita_rope_table: cos/sin tables, bf16 [n, dim/2], for integer positions pos[n] (int64):
 *   freqs = float(pos) * inv_freq[i]  (fp32, like torch.outer),  cos/sin in fp32, cast to bf16
 *   (rotary_pos_embedding.py:200-201 casts cos_/sin_ to t.dtype).  Positions are the *global*
 *   token positions of the local rows, i.e. the zig-zag slice of :36-47 is an index choice.
 * ------------------------------------------------------------------------------------------- */
int vita_rope_table(const int64_t* pos, const float* inv_freq, void* cos_out, void* sin_out,
                    int64_t n, int half_dim, void* stream);

/* cos/sin tables, bf16 [n, half_dim], from the fp32 angles Megatron's RotaryEmbedding.forward returns
 * (`freqs` [s, 1, 1, dim] = cat(freqs, freqs), rotary_pos_embedding.py:106-108; row_stride = dim): the argument
 * apply_rotary_pos_emb(t, freqs, config, cu_seqlens) receives at :232-259.  cos_ = cos(freqs).to(bf16) as :200-201. */
int vita_rope_cos_sin(const float* freqs, int64_t row_stride, void* cos_out, void* sin_out,
                      int64_t n, int half_dim, void* stream);

/* In-place RoPE on a strided [rows, heads, head_dim] bf16 view (non-interleaved halves):
 *   t = bf16(bf16(t*cos) + bf16(rotate_half(t)*sin))   — the rounding chain of :203.
 * row_stride / head_stride in elements.  sign = +1 forward, -1 backward (transpose rotation).
 * Replaces apply_rotary_pos_emb_bshd (M/core/models/common/embeddings/rotary_pos_embedding.py:181-204) on q / k views. */
int vita_rope_apply(void* t, int64_t rows, int heads, int head_dim,
                    int64_t row_stride, int64_t head_stride,
                    const void* cos_tab, const void* sin_tab, int sign, void* stream);

/* Fused RoPE over Megatron's mixed QKV activation [rows, groups, (qpg + 2) * d]
 * (layout: L/core/models/vision/intern_vit_model.py:145-197; weights R/tools/hf2mcore_long_vita.py:597-609):
 * rotates the qpg query heads and the key head of every group in place and, when kv_out != NULL,
 * also packs rotated K and V into kv_out = [kv_split][2][rows][groups / kv_split][d]: kv_split
 * contiguous all-gather messages of the context-parallel attention (split by kv head so that the
 * gather of split j+1 overlaps the attention over split j; kv_split = 1: one message). */
int vita_rope_qkv_fwd(void* mixed_qkv, int64_t rows, int groups, int q_per_group, int head_dim,
                      const void* cos_tab, const void* sin_tab, void* kv_out, int kv_split,
                      void* stream);
/* Backward of the rotation on the gradient of the mixed QKV activation (in place): applies the
 * transpose rotation to the dQ and dK heads, leaves dV untouched.
 * The autograd of apply_rotary_pos_emb_bshd (rotary_pos_embedding.py:181-204) on the mixed QKV gradient. */
int vita_rope_qkv_bwd(void* d_mixed_qkv, int64_t rows, int groups, int q_per_group, int head_dim,
                      const void* cos_tab, const void* sin_tab, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row gather / scatter with int64 indices (bit-exact data movement).
 * Replaces: VocabParallelEmbedding lookup M/core/tensor_parallel/layers.py:216-232;
 *           visual-token scatter M/core/models/common/embeddings/language_model_embedding.py:123,126,131;
 *           masked_select / masked_scatter of the logits-masked head M/core/tensor_parallel/layers.py:348,407,451,455.
 *   gather : dst[i, :] = src[idx[i], :]            i in [0, n)
 *   scatter: dst[dst_idx[i], :] = src[src_idx ? src_idx[i] : i, :]
 * Out-of-range indices set *err_flag (int32 device word, may be NULL) to 1 and are skipped.
 * ------------------------------------------------------------------------------------------- */
int vita_row_gather(const void* src, int64_t src_rows, const int64_t* idx, void* dst,
                    int64_t n, int cols, int elem_bytes, int* err_flag, void* stream);
int vita_row_scatter(const void* src, int64_t src_rows, const int64_t* src_idx,
                     void* dst, int64_t dst_rows, const int64_t* dst_idx,
                     int64_t n, int cols, int elem_bytes, int* err_flag, void* stream);

/* Ordered compaction of a boolean mask: idx_out[k] = position of the k-th true entry,
 * *count_out = number of true entries (device int64).  This is the index form of
 * torch.masked_select (layers.py:348,407).  n <= 2^31. */
int vita_mask_to_index(const uint8_t* mask, int64_t n, int64_t* idx_out, int64_t* count_out,
                       void* stream);

/* Zig-zag context-parallel index remap, the integer arithmetic of
 * M/training/utils.py:279-325,347-350 (get_batch_on_this_cp_rank + index_of_a_in_b):
 *   indices_s [n_img, tok_per_img] int64 global positions -> per element
 *   hit[n_img*tok] (uint8: position owned by this rank) and local[n_img*tok] (int64 local
 *   position after the zig-zag slice, or -1).  seq_len % (2*cp) == 0. */
int vita_cp_index_remap(const int64_t* indices_s, int64_t n, int64_t seq_len, int cp_size,
                        int cp_rank, uint8_t* hit, int64_t* local_pos, void* stream);
/* out[r] = any(mask[r, :])  — `selected_i = torch.any(mask, dim=1)` (M/training/utils.py:284,297). */
int vita_rows_any(const uint8_t* mask, int64_t rows, int cols, uint8_t* out, void* stream);
/* inv[idx[k]] = k  — renumbering of the selected images (utils.py:300 `arange(num_images)`). */
int vita_index_inverse(const int64_t* idx, int64_t n, int64_t* inv, void* stream);
/* For the k-th hit f = hit_idx[k] (flat index into [n_img, tok_per_img]):
 *   src_b = img_rank[f / tok], src_s = f % tok   (utils.py:300-304)
 *   tgt_b = indices_b[f],       tgt_s = local_pos[f]   (utils.py:306-309). */
int vita_cp_src_tgt(const int64_t* hit_idx, int64_t n_hit, int tok_per_img,
                    const int64_t* img_rank, const int64_t* indices_b, const int64_t* local_pos,
                    int64_t* src_b, int64_t* src_s, int64_t* tgt_b, int64_t* tgt_s, void* stream);

/* ---------------------------------------------------------------------------------------------
 * bf16 GEMM on MFMA:   C[M,N] = epilogue(A[M,K] @ W[N,K]^T)        fp32 accumulation.
 * W is row-major [N, K] exactly as torch.nn.Linear / Megatron store it, so this replaces
 * torch.matmul(total_input, weight.t()) (M/core/tensor_parallel/layers.py:270,409), the TE
 * linears of M/core/models/gpt/gpt_layer_specs.py:39-49, the ViT linears and the projector MLP
 * (M/core/models/vision/multimodal_projector.py:53-69).
 *   lda / ldw / ldc / ldr : row strides in elements.  K % 64 == 0, K >= 64; M, N arbitrary.
 * Epilogues (v = fp32 accumulator; every arrow rounds to bf16 like the unfused reference chain):
 *   VITA_EPI_NONE              C = bf16(v)
 *   VITA_EPI_BIAS              C = bf16(v + bias[n])
 *   VITA_EPI_BIAS_GELU         C = bf16(gelu_erf(bf16(v + bias[n])))              (bias may be NULL)
 *   VITA_EPI_RESIDUAL          C = bf16(R[m,n] + bf16(v + bias[n]))               (bias may be NULL)
 *   VITA_EPI_BIAS_SCALE_RES    C = bf16(R[m,n] + bf16(bf16(v + bias[n]) * scale[n]))   (LayerScale,
 *                              M/core/models/vision/intern_vit_model.py:63,77)
 *   VITA_EPI_BIAS2_GELU_TANH   C = bf16(gelu_tanh(bf16(bf16(v) + bias[n])))     (SigLIP MLP: linear_fc1 returns its
 *                              bias unfused (skip_bias_add), M/core/models/vision/siglip_vit_model.py:66-69)
 *   VITA_EPI_BIAS2_RES         C = bf16(R[m,n] + bf16(bf16(v) + bias[n]))        (SigLIP linear_proj / linear_fc2, :50-52,69-72)
 *   VITA_EPI_BIAS2_GELU        C = bf16(gelu_erf(bf16(bf16(v) + bias[n])))      (InternViT MLP under Megatron's local spec: linear_fc1 is
 *                              skip_bias_add and `bias_activation_fusion` is off, M/pretrain_long_vita.py:213 — MLP.forward adds
 *                              the bias to the bf16 product as an op of its own before F.gelu)
 *   VITA_EPI_SWIGLU            W holds [gate(N) ; up(N)] = 2N rows (fc1 = cat[gate, up],
 *                              R/tools/hf2mcore_long_vita.py:612); C[M,N] = bf16(bf16(silu(bf16(g))) * bf16(u))
 * ------------------------------------------------------------------------------------------- */
#define VITA_EPI_NONE 0
#define VITA_EPI_BIAS 1
#define VITA_EPI_BIAS_GELU 2
#define VITA_EPI_RESIDUAL 3
#define VITA_EPI_BIAS_SCALE_RES 4
#define VITA_EPI_SWIGLU 5
#define VITA_EPI_BIAS2_GELU_TANH 6
#define VITA_EPI_BIAS2_RES 7
#define VITA_EPI_BIAS2_GELU 8

int vita_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                   int64_t M, int64_t N, int64_t K, int epilogue, const void* bias,
                   const void* scale, const void* R, int64_t ldr, void* stream);

/* vita_gemm_bf16 on M rows TAKEN OUT of a call over M_select >= M rows: the kernel is chosen as that call chooses it (the 256 x 256 or
 * the 128 x 128 tile, by the tile count of M_select rows), so every row passes through the accumulation order it has there and comes out
 * with the same bits.  M may be smaller than a tile and no multiple of it: rows behind M are neither read nor written.  For the per-row
 * tail of a decoder layer on the rows a logit mask keeps (M/inference/text_generation/generation.py:123-205 keeps one row of a
 * prefill; M/core/models/multimodal/gpt_vl_model.py:339-347 reads only those).  M_select < M: VITA_ERR_INVALID_ARG. */
int vita_gemm_bf16_select(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                          int epilogue, const void* bias, const void* scale, const void* R, int64_t ldr, int64_t M_select,
                          void* stream);

/* The weight-gradient GEMM without transposes (r03): C[M, N] = A_t^T W_t, BOTH operands contraction-major — A_t [K, M] (row stride
 * lda), W_t [K, N] (ldw).  grad_weight = grad_output.t().matmul(total_input) (M/core/tensor_parallel/layers.py:522-523) is exactly this
 * with A_t = grad_output [tokens, out], W_t = total_input [tokens, in] as the forward left them: no vita_transpose_bf16 pass over
 * either.  M, N multiples of 256, K of 64 (VITA_ERR_UNSUPPORTED otherwise: the caller falls back to vita_transpose_bf16 + vita_gemm_bf16). */
int vita_gemm_bf16_tn(const void* At, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N,
                      int64_t K, void* stream);

/* Skinny-M GEMM for the logits-masked LM head (n_sel rows, M <= 16):
 *   logits[M, N] fp32-accumulated, stored bf16 (out_f32 == 0) or fp32 (out_f32 != 0).
 * Replaces torch.matmul on the masked rows, M/core/tensor_parallel/layers.py:402-409. */
/* ABI 16: C[M, N] = A W with A [M, K] row-major and W [K, N] contraction-major — the input-gradient GEMM
 * `grad_input = grad_output.matmul(weight)` (M/core/tensor_parallel/layers.py:444,453) with the weight [out, in] exactly as the forward holds
 * it: no transposed copy.  M, N multiples of 256, K a multiple of 64, rows 16-byte aligned; other shapes: VITA_ERR_UNSUPPORTED (the caller
 * transposes and uses vita_gemm_bf16). */
int vita_gemm_bf16_nn(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                      void* stream);

/* ABI 15: vita_gemm_bf16_tn with the contraction cut into `splits` ranges — for weight gradients whose output is only a few 256 x 256
 * tiles over a long token contraction (the ViT's linears; the decoder's narrow qkv / proj gradients).  Every (split, tile) workgroup
 * writes an fp32 partial to `workspace` ([splits][M][N] floats, vita_gemm_tn_splitk_workspace_bytes), a second kernel sums the splits and
 * rounds once to bf16.  splits <= 1: vita_gemm_bf16_tn.  K / 64 K-tiles are dealt ceil(K / 64 / splits) per split. */
size_t vita_gemm_tn_splitk_workspace_bytes(int64_t M, int64_t N, int splits);
int vita_gemm_bf16_tn_splitk(const void* At, int64_t lda, const void* Wt, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N,
                             int64_t K, int splits, void* workspace, void* stream);
/* ABI 15: out[c] += sum over rows of float(x[r][c]) — grad_bias = grad_output.sum(dim=0) (M/core/tensor_parallel/layers.py:524) in one
 * pass over grad_output.  out: fp32 [cols], zeroed by the caller; cols % 4 == 0. */
int vita_colsum_bf16(const void* x, int64_t ldx, float* out, int64_t rows, int cols, void* stream);
/* ABI 18: the same sums added in a FIXED order — bit-reproducible from run to run, as the reference's grad_output.sum(dim=0) is (the form
 * above adds its row blocks with fp32 atomics, in arrival order).  workspace: vita_colsum_workspace_bytes(rows, cols) bytes, 16-byte aligned;
 * out: fp32 [cols], 16-byte aligned, zeroed (or holding a running sum) on entry. */
size_t vita_colsum_workspace_bytes(int64_t rows, int cols);
int vita_colsum_bf16_ordered(const void* x, int64_t ldx, float* out, int64_t rows, int cols, void* workspace, void* stream);

int vita_gemm_skinny_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, void* C,
                          int64_t ldc, int M, int64_t N, int64_t K, int out_f32, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Flash attention forward (online softmax, fp32 statistics, bf16 I/O), head_dim 64, 96 or 128 (96: SigLIP's 72 zero-padded by the
 * caller, M/core/models/vision/siglip_vit_model.py:29-86; anything else: VITA_ERR_UNSUPPORTED).
 * Replaces flash_attn_func (ViT, M/core/transformer/dot_product_attention.py:318-326),
 * transformers._flash_attention_forward (LLM CP=1, :374-390) and TransformerEngine's
 * AttnFuncWithCP ring (LLM CP>1, M/core/models/gpt/gpt_layer_specs.py:40).
 *
 * Sequence geometry is described by *chunks* so that one kernel serves plain causal, non-causal
 * and zig-zag context-parallel attention:
 *   - the local Q rows are n_q_chunks chunks of chunk_len rows, chunk i carrying the global
 *     chunk id q_chunk_gid[i];
 *   - the K/V rows visible to this rank are n_kv_chunks chunks of chunk_len rows; chunk j starts
 *     at row kv_chunk_row[j] of the K / V buffers and carries global chunk id kv_chunk_gid[j];
 *   - causal != 0: query (gq, i) attends key (gk, j) iff gk < gq or (gk == gq and j <= i);
 *     causal == 0: everything is visible; kv_valid (<= chunk_len) masks the padded tail of a
 *     single-chunk sequence (ViT: 1025 tokens).
 * q/k/v/o strides are in elements; `batch` replicates the geometry (ViT frames).
 * GQA: query head h uses kv head h / (n_q_heads / n_kv_heads); with G = n_q_heads / n_kv_heads the
 * address of query head (g, j) is q + g * q_group_stride + j * q_head_stride (q_group_stride == 0
 * means G * q_head_stride) so Q can be read in place from Megatron's mixed QKV activation;
 * o_group_stride likewise.
 * lse (fp32 [batch, n_q_heads, n_q_rows], natural log) may be NULL.
 * All tables are HOST pointers (<= 64 chunks); they are copied into kernel arguments.
 * Alignment (anything else is VITA_ERR_UNSUPPORTED, refused before a launch): q / k / v 16-byte aligned with every stride a multiple
 * of 8 elements (16-byte loads); o 8-byte aligned with every stride a multiple of 4 elements (8-byte stores); lse and q_seg_start
 * 4-byte aligned.  An o that is also 16-byte aligned with strides of 8 elements takes the 64-row kernels where the geometry allows
 * them; the others run on the general kernel.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q; int64_t q_batch_stride, q_row_stride, q_head_stride, q_group_stride;
  const void* k; int64_t k_batch_stride, k_row_stride, k_head_stride;
  const void* v; int64_t v_batch_stride, v_row_stride, v_head_stride;
  void* o;       int64_t o_batch_stride, o_row_stride, o_head_stride, o_group_stride;
  float* lse;
  int batch, n_q_heads, n_kv_heads, head_dim;
  int64_t chunk_len;        /* rows per chunk                                             */
  int64_t q_valid;          /* valid rows of the last q chunk  (<= chunk_len)             */
  int64_t kv_valid;         /* valid rows of the last kv chunk (<= chunk_len)             */
  int n_q_chunks, n_kv_chunks;
  const int32_t* q_chunk_gid;      /* host [n_q_chunks]  */
  const int32_t* kv_chunk_gid;     /* host [n_kv_chunks] */
  const int64_t* kv_chunk_row;     /* host [n_kv_chunks] */
  int causal;
  float softmax_scale;
  const int32_t* q_seg_start;      /* DEVICE [rows] or NULL: packed sequences (flash_attn_varlen_func with
                                      cu_seqlens, M/core/transformer/dot_product_attention.py:334-367): first row of
                                      the segment each query row belongs to; keys before it are masked.  Needs
                                      batch 1, causal, single-chunk geometry. */
} vita_attn_params;

int vita_flash_attn_fwd(const vita_attn_params* p, void* stream);

/* The same attention for a WINDOW of query tiles: q_tiles (HOST, n_q_tiles distinct indices, any order, at most 32) names 256-row
 * tiles of the query rows (tile t = rows 256 t .. 256 t + 255); only their workgroups are launched, heaviest first, and O (and lse)
 * are written for their rows alone, at their usual addresses.  Each workgroup is the one vita_flash_attn_fwd runs for that tile — the
 * same kernel, rows, key walk and masks — so those rows carry the bits of the full launch.  For the last decoder layer of a prefill
 * whose logit mask keeps a few rows (the decode loop keeps one, M/inference/text_generation/generation.py:123-205): K / V of every row
 * still exist, attention is needed for the kept rows only.  Plain causal geometry of one chunk (n_q_chunks = n_kv_chunks = 1),
 * head_dim 128; anything else: VITA_ERR_UNSUPPORTED (the caller runs the full launch).  A tile out of range or listed twice:
 * VITA_ERR_INVALID_ARG. */
int vita_flash_attn_fwd_window(const vita_attn_params* p, const int32_t* q_tiles, int n_q_tiles, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention of t >= 1 NEW tokens behind a KV cache that already holds their rotated K / V rows (attn_extend.hip): a follow-up turn or
 * one chunk of a chunked prefill.  Replaces the q_len > 1 step behind a DynamicCache of
 * H/models/long_vita_qwen2_intern/modeling_long_vita.py:150-202 (cache_position = arange(past_seen, past_seen + s)) and the cached
 * decode loop M/inference/text_generation/generation.py:127-131 fed more than one token (per-token passes before).
 *   q: t rows read in place from the mixed QKV activation: head j of kv group g of row i at q + i * q_row_stride + g * q_group_stride
 *      + j * q_head_stride.  k_cache / v_cache: rows [0, n_keys) of a cache shard [rows][n_kv_heads][128] (row / group strides in
 *      elements, shared by K and V); rows behind n_keys are never read.  out [t][n_q_heads][128] through its strides; lse (optional)
 *      fp32 [n_q_heads][t], natural log.  head_dim 128 only; q / k_cache / v_cache / out 16-byte aligned, every stride a multiple of
 *      8 elements, lse 4-byte aligned (else VITA_ERR_UNSUPPORTED).
 *   Visibility by position: query row i sits at q_pos0 + i.  Keys [0, n_full) are visible to every row; key k >= n_full sits at
 *      key_pos0 + (k - n_full) * key_pos_step and is visible iff that position <= the row's.  One device, one cache: n_full = the
 *      cached length L, key_pos0 = q_pos0 = L, step 1; step > 1 describes a round-robin shard of the appended rows.  A row that sees no
 *      key returns zeros and lse = -inf.
 *   The keys are cut into splits (a function of t, n_q_heads and n_keys only) so that a short t behind a long cache fills the chip;
 *      with more than one split the launch needs vita_flash_attn_extend_workspace_bytes of device memory (16-byte aligned, contents
 *      ignored; 0 bytes = one split, workspace may be NULL) for the fp32 partials that a merge kernel folds.  Arguments are checked
 *      before anything is launched. */
typedef struct {
  const void* q; int64_t q_row_stride, q_group_stride, q_head_stride;
  const void* k_cache; const void* v_cache; int64_t kv_row_stride, kv_group_stride;
  void* out; int64_t out_row_stride, out_head_stride;
  float* lse;
  int64_t t, n_keys, n_full;
  int64_t q_pos0, key_pos0, key_pos_step;
  int n_q_heads, n_kv_heads, head_dim;
  float softmax_scale;
  void* workspace; size_t workspace_bytes;
} vita_attn_extend_params;
size_t vita_flash_attn_extend_workspace_bytes(int64_t t, int n_q_heads, int64_t n_keys);
int vita_flash_attn_extend_fwd(const vita_attn_extend_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Context-parallel core attention for callers without PyTorch (cp_attn.hip): the K/V exchange of one decoder layer over
 * RCCL + the zig-zag chunk-table attention.  Replaces TransformerEngine's AttnFuncWithCP (the core_attention of
 * M/core/models/gpt/gpt_layer_specs.py:40 under --context-parallel-size > 1: a CP-1-step P2P ring) with one all-gather per
 * kv-head split issued up front on a communication stream — xGMI is point to point, every peer pushes over its own link —
 * and, in the backward, one reduce-scatter of dK / dV per split.  Rank r owns zig-zag chunks {r, 2 CP - 1 - r} of the
 * sequence (M/training/utils.py:329-341); s_local = the two chunks together.
 *
 * vita_cp_unique_id / vita_cp_init / vita_cp_destroy: the RCCL communicator of the context-parallel group (ncclGetUniqueId on
 *   one rank, shipped to the others by any channel, then ncclCommInitRank), the communication stream and its events.  The only
 *   persistent state of the library (SURVEY.md §8b "Ownership"); RCCL is resolved at run time, so nothing here is needed —
 *   or loaded — on the single-GPU path.  cp_size = 1 is valid (the exchange degenerates to a copy through RCCL).
 *   unique_id128 = NULL creates a context WITHOUT a communicator ("external exchange"): the host moves the shards itself (its own
 *   transport — e.g. peer copies on the copy engines — or one process simulating the ranks): vita_cp_attn_fwd then expects
 *   `workspace` to hold the gathered K/V [n_split][cp_size][2][s_local][n_kv_heads / n_split][head_dim] (ordered before `stream`;
 *   its own slot may be left unwritten when scratch enables own-chunks-first) and vita_cp_attn_bwd leaves the reduction of
 *   p->dkv_workspace over the ranks to the caller.
 * vita_cp_attn_fwd: q = this rank's rotated queries as a grouped view (head h of kv group g at q + row * q_row_stride +
 *   g * q_group_stride + h * q_head_stride); kv_packed = its rotated K and V packed [n_split][2 (K | V)][s_local][n_kv_heads /
 *   n_split][head_dim] (what vita_rope_qkv_fwd writes); out [s_local][n_q_heads][head_dim] via out_row/head_stride; lse
 *   (optional) [n_q_heads][s_local].  workspace = vita_cp_attn_workspace_bytes(...) of device memory, caller-owned: the gathered
 *   K/V; it is the `k`/`v` of the backward.  Everything is stream-ordered behind `stream`.
 *   Own chunks first (what TransformerEngine's ring does with its local block): gathers 1.. run under the attention of
 *   the split before them, gather 0 has nothing in front of it.  With p->scratch = vita_cp_attn_scratch_bytes(...) of device
 *   memory (one split's output + two lse vectors) and cp_size > 1, split 0 attends to the rank's OWN two chunks straight from
 *   kv_packed while gather 0 is in flight, then to the 2 CP - 2 remote chunks, and vita_attn_merge joins the two partials;
 *   scratch = NULL keeps one launch per split behind its gather.
 *   Choosing n_split: every split is one attention launch over n_q_heads / n_split heads x s_local / 256 row tiles, one workgroup
 *   per CU, and short launches waste their last round: at s_local = 16384, 40 : 8 heads (2560 workgroups per layer) 1 / 2 / 4 splits
 *   take 18.0-18.3 / 18.8-19.0 / 18.9-19.9 ms per layer (profiles/r03_cp8_rank_attn.jsonl); the host mirror keeps >= 2560
 *   workgroups per launch (long_vita_amd.ops.cp_kv_split).
 * vita_cp_attn_bwd: d_out like out; lse from the forward; delta from vita_attn_delta; dq like q; dkv_packed like kv_packed
 *   receives this rank's dK / dV; p->dkv_workspace (same size as workspace) takes the gathered-layout dK / dV. */
typedef struct vita_cp_context vita_cp_context;
typedef struct {
  const void* q; int64_t q_row_stride, q_head_stride, q_group_stride;
  const void* kv_packed;
  void* out; int64_t out_row_stride, out_head_stride;
  float* lse;
  int64_t s_local;
  int n_q_heads, n_kv_heads, head_dim, n_split;
  float softmax_scale;
  void* workspace; size_t workspace_bytes;
  void* dkv_workspace;
  void* scratch; size_t scratch_bytes;      /* optional (ABI 13): vita_cp_attn_scratch_bytes(...) enables "own chunks first" */
} vita_cp_attn_params;
int vita_cp_unique_id(void* id_out128);
int vita_cp_init(vita_cp_context** ctx, int cp_size, int cp_rank, const void* unique_id128);
int vita_cp_destroy(vita_cp_context* ctx);
size_t vita_cp_attn_workspace_bytes(int cp_size, int64_t s_local, int n_kv_heads, int head_dim);
size_t vita_cp_attn_scratch_bytes(int64_t s_local, int n_q_heads, int n_split, int head_dim);
int vita_cp_attn_fwd(vita_cp_context* ctx, const vita_cp_attn_params* p, void* stream);
int vita_cp_attn_bwd(vita_cp_context* ctx, const vita_cp_attn_params* p, const void* d_out, const float* lse,
                     const float* delta, void* dq, void* dkv_packed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ViT front / back ends.
 * vita_patchify14: im2col of the 14x14 / stride-14 patch conv (M/core/models/vision/intern_vit_model.py:139-145,203-205):
 *   images [n, 3, H, W] bf16 -> patches [n * (H/14) * (W/14), k_pad] bf16, column = c*196 + dy*14 + dx
 *   (the flattening of Conv2d.weight [out, 3, 14, 14]); columns 588..k_pad-1 are zero.
 * vita_vit_assemble: x[n, 1 + P, h] = cat(cls, patch_embeds[n, P, h]) + pos[1 + P, h]   (:207-216),
 *   rounding bf16 after the add.
 * vita_pixel_shuffle_ln: drop cls, pixel-shuffle x0.5 and LayerNorm(4*h) in one pass
 *   (M/pretrain_long_vita.py:467-483,572-582 + :443-446):
 *   x [n, 1 + g*g, h] -> y [n, (g/2)*(g/2), 4h].
 * ------------------------------------------------------------------------------------------- */
int vita_patchify14(const void* images, void* patches, int64_t n, int H, int W, int k_pad,
                    void* stream);
int vita_vit_assemble(const void* patch_embeds, const void* cls_token, const void* pos_emb,
                      void* x, int64_t n, int n_patches, int hidden, int has_cls, void* stream);
int vita_pixel_shuffle_ln(const void* x, const void* w, const void* b, void* y, int64_t n,
                          int grid, int hidden, int has_cls, float eps, void* stream);

/* ABI 15 — the same front / back end under Megatron's module seams (InternViTModel.forward / SigLIPViTModel.forward,
 * M/core/models/vision/intern_vit_model.py:190-261, siglip_vit_model.py:165-228; MegatronVisionModel.forward_downsample /
 * forward_projection, M/pretrain_long_vita.py:436-483), forward AND backward (stage 2 trains the encoder, the projector always trains):
 *   vita_patchify14_ex    token_major != 0: patch row = patch * n + image — Megatron's [s, b, h] order, so the conv GEMM's output IS
 *                         rows 1.. of the encoder input and the backward's gradient rows line up with the patch rows (no transposes).
 *   vita_vit_assemble_ex  token_major as above for patch_embeds and x; pos_row0 = first row of the position table that is looked up
 *                         (InternViTModel without a class token uses rows 1 .. seq, :141-143).
 *   vita_vit_assemble_bwd d_pos[seq, h] = bf16(sum over images of dx[., s, :]) (fp32 sums) — the position table's gradient; its row 0
 *                         is also the class token's (x[:, 0] = cls + pos[0]).
 *   vita_pixel_shuffle_ln_ex   x addressed as x[image * img_stride + token * tok_stride + c] (elements, multiples of 8): the
 *                         contiguous [n, seq, h] tensor or the permuted view of the encoder's [s, b, h] output (no copy);
 *                         norm == 0: the pure permutation (forward_downsample alone; w / b unused).
 *   vita_pixel_shuffle_ln_bwd  dx (x's strides; NULL = frozen encoder; the class token's row receives zeros) and, norm != 0,
 *                         dgamma / dbeta (fp32 [4 h], accumulated: caller zeroes).  4 h <= 4096. */
int vita_patchify14_ex(const void* images, void* patches, int64_t n, int H, int W, int k_pad, int token_major, void* stream);
int vita_vit_assemble_ex(const void* patch_embeds, const void* cls_token, const void* pos_emb, void* x, int64_t n, int n_patches,
                         int hidden, int has_cls, int pos_row0, int token_major, void* stream);
int vita_vit_assemble_bwd(const void* dx, void* d_pos, int64_t n, int seq, int hidden, int token_major, void* stream);
int vita_pixel_shuffle_ln_ex(const void* x, const void* w, const void* b, void* y, int64_t n, int grid, int hidden, int has_cls,
                             float eps, int norm, int64_t img_stride, int64_t tok_stride, void* stream);
int vita_pixel_shuffle_ln_bwd(const void* dy, const void* x, const void* w, void* dx, float* dgamma, float* dbeta, int64_t n,
                              int grid, int hidden, int has_cls, float eps, int norm, int64_t img_stride, int64_t tok_stride,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward pass (training step, reference: torch autograd over the forward modules; the only
 * first-party backward code is M/core/tensor_parallel/layers.py:416-534).
 * ------------------------------------------------------------------------------------------- */

/* dst[c][r] = src[r][c] (bf16).  Used to feed dgrad / wgrad to vita_gemm_bf16, whose operands are
 * both contraction-contiguous:  dX = dY @ W  = gemm(dY, W^T),   dW = dY^T @ X = gemm(dY^T, X^T)
 * (grad_input = grad_output.matmul(weight), grad_weight = grad_output.t().matmul(total_input):
 * layers.py:444, :522-523). */
int vita_transpose_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows,
                        int64_t cols, void* stream);

/* RMSNorm backward of vita_rmsnorm_fwd's expression: dx bf16 (+ `res` when not NULL: the gradient
 * arriving through the residual connection, dx = bf16(res + bf16(dx_norm))); dw_acc fp32 [cols] is
 * ACCUMULATED (caller zeroes it; may be NULL).
 * The autograd of RMSNorm._norm / forward (M/core/transformer/custom_layers/transformer_engine.py:74-79). */
int vita_rmsnorm_bwd(const void* dy, const void* x, const void* w, const void* res, void* dx,
                     float* dw_acc, int64_t rows, int cols, float eps, void* stream);

/* SwiGLU on the unfused fc1 output y = [gate | up] ([rows, 2*ffn]):  a = bf16(bf16(silu(g)) * u);
 * backward writes dy = [dgate | dup].
 * Megatron MLP's `silu(gate) * up` under `--swiglu` (the MLP the spec of M/core/models/gpt/gpt_layer_specs.py:93-104 builds) and its autograd. */
int vita_swiglu_fwd(const void* y, void* a, int64_t rows, int ffn, void* stream);
int vita_swiglu_bwd(const void* y, const void* da, void* dy, int64_t rows, int ffn, void* stream);

/* dx = bf16(dy * gelu_erf'(x)) over n elements (projector MLP, multimodal_projector.py:53-69). */
int vita_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);

/* LayerNorm parameter gradients (projector pre-norm, M/pretrain_long_vita.py:443-446; its input is the
 * frozen ViT's output, so no dx):  dgamma += sum_rows dy*xhat, dbeta += sum_rows dy (fp32, accumulated).
 * prenormalized != 0: x already holds xhat (e.g. vita_pixel_shuffle_ln run with w = 1, b = 0). */
int vita_layernorm_param_grad(const void* dy, const void* x, float* dgamma, float* dbeta,
                              int64_t rows, int cols, float eps, int prenormalized, void* stream);

/* ViT training (reference stage 2 trains the encoder: R/scripts/megatron/qwen25/finetune_..._stage2.sh has no --vision-model-freeze).
 * vita_layernorm_bwd: backward of torch.nn.LayerNorm / TENorm (the block norms of InternViTTransformerLayer,
 *   M/core/models/vision/intern_vit_model.py:46,72): dx, and dgamma / dbeta accumulated into fp32 [cols] (caller zeroes).
 * vita_gelu_fwd: a = bf16(gelu(x)) as a kernel of its own (training keeps the pre-activation for vita_gelu_bwd);
 *   tanh_form != 0: the tanh approximation (SigLIP).
 * vita_bias_scale_res_fwd / _bwd: `hidden = residual + (out + bias) * ls` of InternViTTransformerLayer.forward (:60-66, :79-82)
 *   with a bf16 rounding after each of the three ops, bias / scale optional (NULL); backward: dx = bf16(g * scale),
 *   d_bias += sum_rows dx, d_scale += sum_rows g * bf16(x + bias) (fp32 [cols], caller zeroes; either may be NULL);
 *   d(residual) = g. */
int vita_layernorm_bwd(const void* dy, const void* x, const void* w, void* dx, float* dgamma, float* dbeta,
                       int64_t rows, int cols, float eps, void* stream);
int vita_gelu_fwd(const void* x, void* a, int64_t n, int tanh_form, void* stream);
/* ABI 14: dx = bf16(dy * gelu_tanh'(x)) — the backward of `partial(F.gelu, approximate="tanh")`, SigLIP's activation
 * (M/pretrain_long_vita.py:290; SigLIPViTTransformerLayer's MLP, M/core/models/vision/siglip_vit_model.py:29-86). */
int vita_gelu_tanh_bwd(const void* x, const void* dy, void* dx, int64_t n, void* stream);
int vita_bias_scale_res_fwd(const void* x, const void* bias, const void* scale, const void* residual, void* out,
                            int64_t rows, int cols, void* stream);
int vita_bias_scale_res_bwd(const void* g, const void* x, const void* bias, const void* scale, void* dx, float* d_bias,
                            float* d_scale, int64_t rows, int cols, void* stream);

/* Vocabulary cross-entropy of the selected rows (TP = 1 form of Megatron's vocab-parallel CE, called at
 * M/core/models/multimodal/gpt_vl_model.py:414):  loss[i] = logsumexp(float(logits[i])) - logits[i, label[i]];
 * when dlogits != NULL also dlogits[i] = bf16((softmax - onehot) * grad_scale[i]) (grad_scale NULL = 1).
 * A label outside [0, vocab) (the datasets pad with IGNORE_TOKEN_ID = -100, M/pretrain_long_vita.py:751) is treated as Megatron's
 * vocab_parallel_cross_entropy treats it — masked target: loss[i] = log sum exp(logits[i] - max), no one-hot term in dlogits[i] — and
 * additionally sets *err_flag when err_flag != NULL (ABI 17; before: the row was skipped). */
int vita_ce_loss(const void* logits, int64_t ld, const int64_t* labels, float* loss, void* dlogits,
                 int64_t ld_d, const float* grad_scale, int64_t rows, int vocab, int* err_flag,
                 void* stream);
/* ABI 15: the same on fp32 logits with fp32 dlogits — what `tensor_parallel.vocab_parallel_cross_entropy(logits.float(), labels)`
 * receives (megatron LanguageModule.compute_language_model_loss, called at gpt_vl_model.py:414); loss may be NULL when only
 * dlogits is wanted (the autograd backward re-runs the row pass with grad_scale = the incoming gradient). */
int vita_ce_loss_f32(const float* logits, int64_t ld, const int64_t* labels, float* loss, float* dlogits,
                     int64_t ld_d, const float* grad_scale, int64_t rows, int vocab, int* err_flag, void* stream);

/* ABI 17: the vocabulary-PARALLEL cross entropy (TP > 1) — megatron.core.tensor_parallel.cross_entropy.vocab_parallel_cross_entropy
 * as LanguageModule.compute_language_model_loss calls it at M/core/models/multimodal/gpt_vl_model.py:414.  Each rank keeps its
 * [rows, vocab_local] shard (logits bf16, or fp32 when is_f32) and its labels in GLOBAL vocabulary ids:
 *   vita_ce_vp_stats   stats[row] = {max, sum exp(l - max), predicted raw logit or 0, 1 if vocab_start <= label < vocab_start + vocab_local};
 *   (caller: all-gather the [rows, 4] fp32 records over the tensor-parallel group -> stats_all [tp, rows, 4], rank-major)
 *   vita_ce_vp_finish  loss[row] = log(sum exp) - (predicted - max), or log(sum exp) when no shard holds the label (masked target);
 *                      row_stat[row] = {global max, global sum exp} for the backward; loss may be NULL;
 *   vita_ce_vp_grad    dlogits[row, v] = (exp(l - max) / sumexp - [v == label - vocab_start]) * grad_scale[row]  (NULL = 1), shard only. */
int vita_ce_vp_stats(const void* logits, int is_f32, int64_t ld, const int64_t* labels, int64_t vocab_start, float* stats,
                     int64_t rows, int vocab_local, void* stream);
int vita_ce_vp_finish(const float* stats_all, int tp, int64_t rows, float* loss, float* row_stat, void* stream);
int vita_ce_vp_grad(const void* logits, int is_f32, int64_t ld, const int64_t* labels, int64_t vocab_start, const float* row_stat,
                    const float* grad_scale, void* dlogits, int64_t ld_d, int64_t rows, int vocab_local, void* stream);

/* dst_f32[idx[i], :] += float(src_bf16[i, :]) — word-embedding weight gradient (the backward of
 * M/core/tensor_parallel/layers.py:216-232); idx[i] < 0 skips row i (visual-token positions). */
int vita_row_scatter_add_f32(const void* src, const int64_t* idx, float* dst, int64_t dst_rows,
                             int64_t n, int cols, int* err_flag, void* stream);

/* ABI 19: the ORDERED (deterministic) forms of the backward's parameter-gradient reductions — the reference's `--use-deter-comp`
 * (M/training/arguments.py:557) and torch.use_deterministic_algorithms(True).  The entries above add each workgroup's column sums
 * into the caller's fp32 buffer with atomics, in arrival order, so two runs can differ in the last bits.  These run the same kernels,
 * with the same per-workgroup arithmetic and the same dx bits, but workgroup b stores its sums to row b of `workspace` and a finish pass
 * adds the rows in ascending block order: acc[c] = ((acc[c] + p0[c]) + p1[c]) + ...  The block count depends on (rows, cols) only,
 * so the bits do not depend on the CU count, occupancy or other work on the device.  Accumulation contract as above (caller zeroes
 * or holds a running sum).  workspace: *_workspace_bytes(rows, cols) bytes (<= 32 MiB), 16-byte aligned, contents ignored; NULL
 * with rows > 0 is VITA_ERR_INVALID_ARG, checked before anything is launched.
 *   vita_rmsnorm_bwd_ordered            vita_rmsnorm_bwd (transformer_engine.py:74-79); dw_acc NULL: no reduction, workspace unused.
 *   vita_layernorm_bwd_ordered          vita_layernorm_bwd (intern_vit_model.py:46,72).
 *   vita_bias_scale_res_bwd_ordered     vita_bias_scale_res_bwd (intern_vit_model.py:60-66,79-82); at most 2048 row blocks.
 *   vita_layernorm_param_grad_ordered   vita_layernorm_param_grad (M/pretrain_long_vita.py:443-446); the four waves of a
 *                                       workgroup are summed in wave order before the store.
 *   vita_pixel_shuffle_ln_bwd_ordered   vita_pixel_shuffle_ln_bwd with norm = 1 (M/pretrain_long_vita.py:467-483 + :443-446);
 *                                       workspace_bytes takes rows = n (grid / 2)^2, cols = 4 hidden. */
size_t vita_rmsnorm_bwd_workspace_bytes(int64_t rows, int cols);
int vita_rmsnorm_bwd_ordered(const void* dy, const void* x, const void* w, const void* res, void* dx, float* dw_acc, int64_t rows, int cols,
                             float eps, void* workspace, void* stream);
size_t vita_layernorm_bwd_workspace_bytes(int64_t rows, int cols);
int vita_layernorm_bwd_ordered(const void* dy, const void* x, const void* w, void* dx, float* dgamma, float* dbeta, int64_t rows, int cols,
                               float eps, void* workspace, void* stream);
size_t vita_bias_scale_res_bwd_workspace_bytes(int64_t rows, int cols);
int vita_bias_scale_res_bwd_ordered(const void* g, const void* x, const void* bias, const void* scale, void* dx, float* d_bias,
                                    float* d_scale, int64_t rows, int cols, void* workspace, void* stream);
size_t vita_layernorm_param_grad_workspace_bytes(int64_t rows, int cols);
int vita_layernorm_param_grad_ordered(const void* dy, const void* x, float* dgamma, float* dbeta, int64_t rows, int cols, float eps,
                                      int prenormalized, void* workspace, void* stream);
size_t vita_pixel_shuffle_ln_bwd_workspace_bytes(int64_t rows, int cols);
int vita_pixel_shuffle_ln_bwd_ordered(const void* dy, const void* x, const void* w, void* dx, float* dgamma, float* dbeta, int64_t n,
                                      int grid, int hidden, int has_cls, float eps, int64_t img_stride, int64_t tok_stride,
                                      void* workspace, void* stream);
/* ABI 19: the ordered word-embedding gradient (the backward of M/core/tensor_parallel/layers.py:216-232) without atomics.  The caller
 * stable-sorts the ids: sorted_idx[k] ascending, order[k] = the row of src holding the k-th entry (rows ascending among equal ids).
 * Each id's rows are summed in row order — long runs in fixed 256-entry chunks whose partials are added in chunk order — and every
 * destination row is written once: dst[id] = dst[id] + sum.  Negative ids are skipped; ids >= dst_rows set *err_flag.  cols % 8 == 0;
 * src / dst / workspace 16-byte aligned; workspace: vita_row_scatter_add_workspace_bytes(n, cols) bytes. */
size_t vita_row_scatter_add_workspace_bytes(int64_t n, int cols);
int vita_row_scatter_add_f32_sorted(const void* src, const int64_t* sorted_idx, const int64_t* order, float* dst, int64_t dst_rows,
                                    int64_t n, int cols, void* workspace, int* err_flag, void* stream);

/* delta[h, row] = sum_d float(dO[row,h,d]) * float(O[row,h,d])  (attention backward pre-pass).
 * First kernel of the flash-attention backward that stands behind M/core/transformer/dot_product_attention.py:374-390. */
int vita_attn_delta(const void* o, const void* d_o, float* delta, int64_t rows, int heads,
                    int head_dim, int64_t o_row_stride, int64_t o_head_stride, int64_t do_row_stride,
                    int64_t do_head_stride, void* stream);

/* Flash attention backward (head_dim 128 | 96 | 64, causal through the chunk tables, batch 1) over the same chunk geometry as
 * vita_flash_attn_fwd (chunk_len % 128 == 0).  q/k/v are the forward's (rotated) inputs, lse its
 * log-sum-exp output [n_q_heads, n_q_rows], delta from vita_attn_delta.  dk/dv are written for EVERY
 * key row of the visible K/V buffer (under context parallelism: the gathered layout, to be
 * reduce-scattered by the caller).
 * Alignment (anything else is VITA_ERR_UNSUPPORTED, refused before a launch): q / k / v / d_o 16-byte aligned with every stride a
 * multiple of 8 elements (16-byte loads); lse / delta / q_seg_start / k_seg_end 4-byte aligned; the outputs a pass writes (dq; dk and
 * dv) 8-byte aligned with every stride a multiple of 4 elements (8-byte stores).  Outputs that are also 16-byte aligned with strides
 * of 8 elements take the 64-row kernels where the geometry allows them; the others run on the general kernels. */
typedef struct {
  const void* q; int64_t q_row_stride, q_head_stride, q_group_stride;
  const void* k; int64_t k_row_stride, k_head_stride;
  const void* v; int64_t v_row_stride, v_head_stride;
  const void* d_o; int64_t do_row_stride, do_head_stride;
  const float* lse;
  const float* delta;
  void* dq; int64_t dq_row_stride, dq_head_stride, dq_group_stride;
  void* dk; int64_t dk_row_stride, dk_head_stride;
  void* dv; int64_t dv_row_stride, dv_head_stride;
  int n_q_heads, n_kv_heads, head_dim;
  int64_t chunk_len;
  int n_q_chunks, n_kv_chunks;
  const int32_t* q_chunk_gid;      /* host */
  const int32_t* kv_chunk_gid;     /* host */
  const int64_t* kv_chunk_row;     /* host */
  float softmax_scale;
  const int32_t* q_seg_start;      /* DEVICE [rows] or NULL: packed sequences, as in vita_attn_params */
  const int32_t* k_seg_end;        /* DEVICE [rows] or NULL: one past the last row of each key row's segment */
} vita_attn_bwd_params;

int vita_flash_attn_bwd(const vita_attn_bwd_params* p, void* stream);
/* ABI 15: the two passes separately — VITA_ATTN_BWD_DKV (dK + dV of every key row: needs p->dk, p->dv) and VITA_ATTN_BWD_DQ
 * (needs p->dq); with both bits dK / dV are launched first.  A context-parallel caller runs DKV, starts the reduce-scatter of
 * dK / dV on its communication stream, then runs DQ under it (vita_cp_attn_bwd; TE's ring does the same with its P2P steps). */
#define VITA_ATTN_BWD_DQ 1
#define VITA_ATTN_BWD_DKV 2
int vita_flash_attn_bwd_parts(const vita_attn_bwd_params* p, int parts, void* stream);

/* Merge of two attention partials over DISJOINT key sets (their natural-log lse from vita_flash_attn_fwd), in place into the first:
 *   lse = log(exp(lse_a) + exp(lse_b)),  O_a = O_a exp(lse_a - lse) + O_b exp(lse_b - lse)      (a part that saw no key: lse = -inf).
 * o_a / o_b [rows, heads, 128] bf16 with row / head strides in elements, lse_a / lse_b [heads, rows] fp32.
 * Context parallelism: a rank attends to its own zig-zag chunks while the K/V all-gather of the first kv-head split is in flight,
 * then to the remote chunks, and merges — replaces the "local block first" step of TransformerEngine's AttnFuncWithCP ring
 * (reached from M/core/models/gpt/gpt_layer_specs.py:40); SURVEY.md 8(e). */
int vita_attn_merge(void* o_a, int64_t oa_row_stride, int64_t oa_head_stride, float* lse_a, const void* o_b,
                    int64_t ob_row_stride, int64_t ob_head_stride, const float* lse_b, int64_t rows, int heads, int head_dim,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * Single-token decode against a sequence-sharded KV cache.
 * The decode loop M/inference/text_generation/generation.py:123-205 with --use-kv-cache feeds
 * tokens[:, prev:ctx] (one token) through the model; under context parallelism the reference turns
 * the cache off (server_cp .sh:184) and re-prefills.  These three kernels are the per-token path:
 *
 * vita_gemv_bf16: y[N] = epilogue(W[N,K] . x[K]) for one token (M = 1) — the linears of
 *   M/core/tensor_parallel/layers.py:825 at sq = 1.  Epilogues NONE / BIAS / RESIDUAL / SWIGLU
 *   (W = cat[gate, up], N = ffn) with the rounding chain of vita_gemm_bf16.
 * vita_decode_attn_partial: the new token's rotated query (qpg heads per kv group, strided view)
 *   against `len` cached rows k_cache/v_cache[len][groups][128] (row / group strides in elements;
 *   len_dev != NULL: the row count is min(len, *len_dev), an int32 in device memory, so that a
 *   captured hipGraph of the token step can be replayed as the cache grows);
 *   n_splits x groups workgroups each write an un-normalised partial: max and sum in the log2
 *   domain part_m, part_l [n_splits][heads] and part_o [n_splits][heads][128] (fp32).
 * vita_decode_attn_merge: merges nparts partials per head (part p at part_m/l + p*part_ml_stride,
 *   part_o + p*part_o_stride, in floats).  out_bf16 != NULL: normalised context
 *   [heads][128] bf16; else the merged partial (out_m, out_l [heads], out_o [heads][128]) that the
 *   ranks exchange (one all-gather of (128+2)*heads floats per layer) and merge again.
 * Replaces the inference branch of Megatron's Attention.forward (_adjust_key_value_for_inference +
 * core attention at sq = 1), which M/core/transformer/dot_product_attention.py:153 is called from. */
int vita_gemv_bf16(const void* x, const void* W, int64_t ldw, void* y, int64_t N, int64_t K,
                   int epilogue, const void* bias, const void* R, void* stream);
int vita_decode_attn_partial(const void* q, int64_t q_group_stride, int64_t q_head_stride,
                             const void* k_cache, const void* v_cache, int64_t kv_row_stride,
                             int64_t kv_group_stride, int len, const void* len_dev, int n_splits,
                             int groups, int qpg, int head_dim, float softmax_scale, void* part_m,
                             void* part_l, void* part_o, void* stream);
int vita_decode_attn_merge(const void* part_m, const void* part_l, const void* part_o, int nparts,
                           int64_t part_ml_stride, int64_t part_o_stride, int heads, int head_dim, void* out_m, void* out_l, void* out_o,
                           void* out_bf16, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Beam search on a shared-prefix KV cache (CP = 1, TP = 1, 2 .. 8 beams).  Replaces the per-step work of
 * beam_search_and_return_on_first_stage, M/inference/text_generation/generation.py:283-471, which repeats the prompt
 * beam_size times, prefills the copies and keeps one cache per copy: here the prompt is prefilled and cached once, the
 * weights and the prompt's K / V are streamed once per step for all beams, and reordering the beams moves no K / V.
 *
 * vita_gemv_rows_bf16: y[b][N] = epilogue(W[N,K] . norm?(x[b][K])) for b < rows <= 8 (x, y, R through their row strides
 *   ldx, ldy, ldr in elements); every weight row is read once for all input rows.  The epilogues of vita_gemv_bf16; bias per
 *   output, residual R per row.  gamma != NULL: x[b] is RMS-normalised first (gamma [K], eps).  Row b has the bits of
 *   vita_gemv_bf16 on row b, with gamma of vita_rmsnorm_fwd followed by vita_gemv_bf16.  rows > 8: VITA_ERR_UNSUPPORTED.
 * vita_beam_attn_fwd: the contexts out [n_beams][n_q_heads][128] (bf16, dense) of the beams' query rows (row b at
 *   q + b * q_row_stride, head j of kv group g at + g * q_group_stride + j * q_head_stride: read in place from the mixed QKV rows).
 *   Beam b sees the prefix rows [0, prefix_len) of k_cache / v_cache (the cache shard of the prompt, strides as for
 *   vita_flash_attn_extend_fwd; read once per kv group for all beams; rows behind prefix_len are never read) and its own
 *   generated tokens in the tail caches k_tail / v_tail [tail_cap][n_beams][n_kv_heads][128] (dense): the key of step s < n_gen
 *   is row s * n_beams + ancestry[b * tail_cap + s] (int32, device).  Every table entry is clamped into [0, n_beams) before it
 *   forms an address; steps >= n_gen and slots no beam names are never read.  The prefix pass (key splits), the tail pass and
 *   one merge exchange un-normalised fp32 partials through the workspace (vita_beam_attn_workspace_bytes, 16-byte aligned);
 *   no intermediate context is rounded to bf16.  n_q_heads / n_kv_heads <= 8, head_dim 128.
 * vita_beam_candidates: bf16 logits [rows][ld] (cols valid columns), fp32 beam_scores [rows]: x = logit / temperature,
 *   score = x - max - log(sum exp(x - max)) + beam_scores[row] in fp32; idx_out / score_out [n_out] = the n_out best of all
 *   rows * cols, as flat index row * cols + col, by descending score, equal scores by ascending flat index.  rows = 1 is the
 *   reference's first step (:369-370, :455-456).  n_out <= 16, rows <= 16.  A temperature that is not positive and finite, or
 *   n_out > rows * cols: VITA_ERR_INVALID_ARG; cols > 2^23: VITA_ERR_UNSUPPORTED.  Nothing is launched on a refusal.
 * M/inference/text_generation/generation.py:283-471 */
int vita_gemv_rows_bf16(const void* x, int64_t ldx, int rows, const void* W, int64_t ldw, void* y, int64_t ldy, int64_t N,
                        int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr, const void* gamma, float eps,
                        void* stream);
/* M/inference/text_generation/generation.py:283-471 */
size_t vita_beam_attn_workspace_bytes(int n_beams, int n_q_heads, int64_t prefix_len);
/* M/inference/text_generation/generation.py:283-471 */
int vita_beam_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_group_stride, int64_t q_head_stride,
                       const void* k_cache, const void* v_cache, int64_t kv_row_stride, int64_t kv_group_stride,
                       int64_t prefix_len, const void* k_tail, const void* v_tail, int64_t tail_cap,
                       const int32_t* ancestry, int n_beams, int n_gen, int n_q_heads, int n_kv_heads, int head_dim,
                       float softmax_scale, void* out, void* workspace, size_t workspace_bytes, void* stream);
/* M/inference/text_generation/generation.py:283-471 */
int64_t vita_beam_candidates_workspace_bytes(int64_t rows, int64_t cols);
/* M/inference/text_generation/generation.py:283-471 */
int vita_beam_candidates(const void* logits /* bf16 [rows, ld] */, int64_t ld, int64_t rows, int64_t cols,
                         const float* beam_scores /* [rows] */, float temperature, int n_out, int64_t* idx_out /* [n_out] */,
                         float* score_out /* [n_out] */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched decode: 2 .. 8 requests advance one token each in ONE step, every request on the bf16 cache its own batch-1 prefill
 * allocated (CP = 1, TP = 1).  Stands behind the loop of generate_tokens_probs_and_return_on_first_stage,
 * M/inference/text_generation/generation.py:33-280, at batch_size > 1: the weights are streamed once per step for all rows
 * (vita_gemv_rows_bf16), and these three entries are the per-row part.  The caches are reached through a pointer table in device
 * memory, kv_ptrs [n_rows][2] of 64-bit addresses (K base, V base of row b's cache [capacity_b][groups][128], bf16); the row and
 * group strides (elements, multiples of 8) are common to all rows, the capacities caps [n_rows] (int32, device) are not.
 *
 * vita_decode_attn_batch_partial: grid (n_splits, groups, n_rows).  Row b's query heads are read in place from row b of the mixed QKV
 *   buffer (q + b * q_row_stride, head j of kv group g at + g * q_group_stride + j * q_head_stride); it attends to the first
 *   min(lens[b], caps[b]) rows of its cache (lens int32 [n_rows], device; the host sizes n_splits from the longest row).  A row's
 *   split geometry follows from its own length: splits_b = min(n_splits, ceil(len_b / 128)) workgroups share its keys, the ones
 *   behind them write the neutral partial, so row b's partials are those of vita_decode_attn_partial with n_splits = splits_b, bit
 *   for bit, whatever the other rows hold.  lens[b] <= 0: an idle row — every split writes the neutral partial and neither its cache
 *   nor its table entry is read.  part_m, part_l [n_rows][n_splits][heads], part_o [n_rows][n_splits][heads][128], fp32.
 * vita_decode_attn_batch_merge: grid (heads, n_rows): out [n_rows][heads][128] bf16, row b merged from its splits_b parts with the
 *   arithmetic of vita_decode_attn_merge in the same order; an idle row is all zero.
 * vita_rope_append_rows: RoPE of the q and k heads of n_rows mixed QKV rows in place (row b at mixed + b * mixed_row_stride, cos / sin
 *   [n_rows][64] bf16: one position per row), and row b's rotated K and its V stored to row append_rows[b] of its cache (int32
 *   [n_rows], device); append_rows[b] < 0 or >= caps[b]: rotated, nothing stored.  The arithmetic of vita_rope_qkv_fwd.
 * Nothing is launched on a refusal: a null pointer, n_rows <= 0, n_splits <= 0, groups <= 0: VITA_ERR_INVALID_ARG; n_rows > 8,
 * n_splits > 128, head_dim != 128, a qpg outside 1 .. 8, a stride that is not a multiple of 8: VITA_ERR_UNSUPPORTED.
 * M/inference/text_generation/generation.py:33-280 */
int vita_decode_attn_batch_partial(const void* q, int64_t q_row_stride, int64_t q_group_stride, int64_t q_head_stride,
                                   const void* kv_ptrs, int64_t kv_row_stride, int64_t kv_group_stride, const int32_t* lens,
                                   const int32_t* caps, int n_rows, int n_splits, int groups, int qpg, int head_dim,
                                   float softmax_scale, void* part_m, void* part_l, void* part_o, void* stream);
/* M/inference/text_generation/generation.py:33-280 */
int vita_decode_attn_batch_merge(const void* part_m, const void* part_l, const void* part_o, const int32_t* lens,
                                 const int32_t* caps, int n_rows, int n_splits, int heads, int head_dim, void* out, void* stream);
/* M/inference/text_generation/generation.py:33-280 */
int vita_rope_append_rows(void* mixed, int64_t mixed_row_stride, int n_rows, int groups, int qpg, int head_dim, const void* cos,
                          const void* sin, const void* kv_ptrs, int64_t kv_row_stride, int64_t kv_group_stride,
                          const int32_t* append_rows, const int32_t* caps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Several continuations of ONE prefilled prompt in one step: 1 .. 8 rows whose first prefix_len tokens are the same (questions
 * about one video), CP = 1, TP = 1.  Stands behind the loop of generate_tokens_probs_and_return_on_first_stage,
 * M/inference/text_generation/generation.py:33-280, at batch_size > 1, which prefills every row over the whole prompt and keeps a
 * cache per row: here the common prefix is prefilled and cached once and read once per kv group and step for all rows.
 *
 * vita_prefix_batch_attn_fwd: the contexts out [n_rows][n_q_heads][128] (bf16, dense) of the rows' query heads (read in place from
 *   the mixed QKV rows, addressed as for vita_beam_attn_fwd).  Row b sees the rows [0, prefix_len) of k_cache / v_cache (strides as
 *   for vita_flash_attn_extend_fwd; never written, rows behind prefix_len never read) and the first
 *   min(max(tail_lens[b], 0), tail_cap) rows of its own bf16 tail [tail_cap][n_kv_heads][128].  tail_ptrs is [n_rows][2] of 64-bit
 *   addresses in device memory (K base, V base of row b's tail, 16-byte aligned): the table of vita_decode_attn_batch_partial, so
 *   one table serves vita_rope_append_rows and this entry; tail_row_stride / tail_group_stride (elements, multiples of 8) are
 *   common to all rows.  tail_lens is int32 [n_rows] in device memory: the host passes no length and reads nothing back.
 *   tail_lens[b] <= 0: an idle row — it gets the attention over the prefix alone, and neither its tail nor its table entry is read.
 *   The prefix pass is vita_beam_attn_fwd's launch, the tail pass runs vita_beam_attn_fwd's tail arithmetic on the row's own keys,
 *   and the merge is the same: row b has the bits of row b of vita_beam_attn_fwd with n_rows beams, an identity ancestry table,
 *   n_gen = tail_lens[b] and the same tail data, whatever the other rows' lengths are.  The workspace
 *   (vita_prefix_batch_attn_workspace_bytes, 16-byte aligned; 0 for a shape the entry refuses) holds the fp32 partials.
 * Nothing is launched on a refusal: a null pointer, n_rows < 1, prefix_len <= 0, a scale that is not positive and finite,
 * tail_cap < 0, a workspace that is too short: VITA_ERR_INVALID_ARG; n_rows > 8, n_q_heads / n_kv_heads > 8, head_dim != 128, a
 * stride that is not a multiple of 8, a base that is not 16-byte aligned: VITA_ERR_UNSUPPORTED.
 * M/inference/text_generation/generation.py:33-280 */
size_t vita_prefix_batch_attn_workspace_bytes(int n_rows, int n_q_heads, int64_t prefix_len);
/* M/inference/text_generation/generation.py:33-280 */
int vita_prefix_batch_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_group_stride, int64_t q_head_stride,
                               const void* k_cache, const void* v_cache, int64_t kv_row_stride, int64_t kv_group_stride,
                               int64_t prefix_len, const void* tail_ptrs, int64_t tail_row_stride, int64_t tail_group_stride,
                               const int32_t* tail_lens, int tail_cap, int n_rows, int n_q_heads, int n_kv_heads, int head_dim,
                               float softmax_scale, void* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The rows' own prompt tokens behind the shared prefix in ONE pass (the rows' questions about one video): what the loop above
 * teacher-forces one token per step, M/inference/text_generation/generation.py:33-280, as vita_flash_attn_extend_fwd does for one
 * request — but a row's keys are not contiguous: the prefix lives in the prefix request's cache, the row's own tokens in its tail.
 *
 * vita_prefix_extend_attn_fwd: the contexts out [n_tokens][n_q_heads][128] (bf16, dense) of n_tokens query rows of the mixed QKV
 *   buffer (addressed as for vita_flash_attn_extend_fwd).  The rows belong to n_rows <= 8 segments, one per continuation row b:
 *   segments is int32 [n_rows][3] in device memory = (first query row, count_b, tail0_b), tail0_b the rows b's tail held before this
 *   pass.  Query i of segment b sees the rows [0, prefix_len) of k_cache / v_cache (never written; rows behind prefix_len never
 *   read) and the rows [0, tail0_b + i] of row b's tail, reached through tail_ptrs / tail_row_stride / tail_group_stride / tail_cap
 *   as in vita_prefix_batch_attn_fwd; the new tokens' rotated K / V are already in the tail at rows [tail0_b, tail0_b + count_b),
 *   and nothing behind them is read.  count_b = 0: an idle row — neither its tail nor its entry of tail_ptrs is read.  A query row
 *   no segment names gets the attention over the prefix alone.  Every triple is clamped on the device before it forms an address:
 *   first into [0, n_tokens], tail0 into [0, tail_cap], count into [0, min(max_count, n_tokens - first, tail_cap - tail0)].
 *   n_tokens and max_count (the largest count) are host arguments: they size the grids.  The prefix pass is
 *   vita_flash_attn_extend_fwd's kernel over the prefix with every key visible (key splits by vita_beam_attn_fwd's rule for n_tokens
 *   rows); the tail pass is ONE launch of the same kernel for all segments (MFMA, the diagonal at the segment's first query) that
 *   writes one more part; the merge is vita_beam_attn_fwd's.  Both passes take two bf16 terms of P while n_tokens * (n_q_heads /
 *   n_kv_heads) <= 256 and one beyond, as vita_flash_attn_extend_fwd does; no intermediate context is rounded to bf16.  The
 *   workspace (vita_prefix_extend_attn_workspace_bytes, 16-byte aligned; 0 for a shape the entry refuses) holds the fp32 partials.
 * Nothing is launched on a refusal and out stays untouched: a null pointer, n_rows < 1, n_tokens < 1, max_count < 0,
 * prefix_len <= 0, a scale that is not positive and finite, tail_cap < 0, a workspace that is too short: VITA_ERR_INVALID_ARG;
 * n_rows > 8, n_tokens > 32768, n_q_heads / n_kv_heads > 8, head_dim != 128, a stride that is not a multiple of 8, a base that is
 * not 16-byte aligned: VITA_ERR_UNSUPPORTED.
 * M/inference/text_generation/generation.py:33-280 */
size_t vita_prefix_extend_attn_workspace_bytes(int64_t n_tokens, int n_q_heads, int64_t prefix_len);
/* M/inference/text_generation/generation.py:33-280 */
int vita_prefix_extend_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_group_stride, int64_t q_head_stride,
                                const void* k_cache, const void* v_cache, int64_t kv_row_stride, int64_t kv_group_stride,
                                int64_t prefix_len, const void* tail_ptrs, int64_t tail_row_stride, int64_t tail_group_stride,
                                int tail_cap, const int32_t* segments, int n_rows, int64_t n_tokens, int max_count, int n_q_heads,
                                int n_kv_heads, int head_dim, float softmax_scale, void* out, void* workspace,
                                size_t workspace_bytes, void* stream);

/* out[n] = bf16(a[n] + b[n]) (n % 8 == 0): the residual add that follows the tensor-parallel all-reduce of a
 * row-parallel linear's output (RowParallelLinear + bias_dropout_add, TP > 1 only; at TP = 1 the add is the GEMM's
 * RESIDUAL epilogue).
 * RowParallelLinear.forward + bias_dropout_add (M/core/tensor_parallel/layers.py:1059-1115). */
int vita_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);

/* One decoder layer for one token, launched from C: vita_decode_layer_attn = RMSNorm (fused into the
 * GEMV) + QKV GEMV + bias -> RoPE + K/V append -> decode attention partial -> merge; vita_decode_layer_mlp
 * = [merge of the CP ranks' partials] -> o-proj GEMV + residual -> RMSNorm + fc1 GEMV + SwiGLU -> fc2 GEMV
 * + residual.  Same kernels and rounding chains as the separate entry points; the split is where the
 * context-parallel all-gather of the packed partial (msg: heads*head_dim + 2*heads floats) sits.
 * Replaces TransformerLayer.forward at sq = 1 (the TE layer spec of M/core/models/gpt/gpt_layer_specs.py:35-49
 * under the decode loop M/inference/text_generation/generation.py:127-131). */
typedef struct {
  const void *ln1, *qkv_w, *qkv_b, *o_w, *ln2, *fc1_w, *fc2_w; /* one layer, Megatron layout, bf16 */
  int hidden, heads, kv_groups, head_dim, ffn;
  float eps, softmax_scale;
  void* h;                       /* [hidden] residual stream, updated in place */
  const void *cos, *sin;         /* [head_dim / 2] bf16 for this token's position */
  void *k_cache, *v_cache;       /* this rank's shard [capacity][kv_groups][head_dim] (strides in elements) */
  int64_t kv_row_stride, kv_group_stride;
  int capacity;
  int append_row;                /* >= 0: row that receives this token's K / V; < 0: another rank owns the token */
  int len;                       /* rows attended to (including the appended one) */
  int n_splits;
  void *qkv, *ctx, *act;         /* scratch: [(heads + 2 kv_groups) head_dim], [heads head_dim], [ffn] bf16 */
  void *part_m, *part_l, *part_o; /* scratch fp32: [n_splits][heads] x 2, [n_splits][heads][head_dim] */
  void* msg;                     /* attn entry, CP > 1: packed partial written here instead of ctx */
  const void* gathered;          /* mlp entry, CP > 1: [n_ranks][heads head_dim + 2 heads] fp32 */
  int n_ranks;
} vita_decode_layer_params;
int vita_decode_layer_attn(const vita_decode_layer_params* p, void* stream);
int vita_decode_layer_mlp(const vita_decode_layer_params* p, void* stream);

/* ---------------------------------------------------------------------------------------------
 * FP8 KV cache for the cached decode (opt-in, CP = 1 and TP = 1).  What Megatron keeps per layer in
 * InferenceParams.key_value_memory_dict (and the HF DynamicCache of modeling_long_vita.py:150-202) as bf16 is kept as OCP e4m3fn
 * codes [capacity][groups][128] (1 byte per element) plus one fp32 scale per (row, kv group) [capacity][groups], K and V apart.
 * The rule, per K (after RoPE) or V head row x[0..127]: amax = max |x_i| (a NaN element makes it NaN); s = amax > 0 ? amax / 448 : 1;
 * code_i = e4m3fn_rne(x_i / s) (fp32, IEEE division, no clamp); the cache reads back f32(code_i) * s.  A non-finite element leaves
 * non-finite values in its row.  Code strides are in BYTES and multiples of 8 (8-byte vectors, pointers 8-byte aligned); scale
 * strides are in floats.
 *
 * vita_kv8_store: quantises `rows` K and V head rows per group, read in place from the mixed qkv buffer (k_src / v_src point at
 *   row 0, group 0; strides in bf16 elements, multiples of 8, pointers 16-byte aligned), into cache rows row0 + r.  row0_dev != NULL:
 *   row0 is read from that int64 in device memory (the captured token step).  A row range that does not lie inside
 *   [0, capacity) writes nothing (refused on the host when row0 is the host's).  Rows outside [row0, row0 + rows) are not touched.
 *   Fills the cache during prefill (rows = s) and appends a decode token (rows = 1).
 * vita_decode_attn_partial_kv8: vita_decode_attn_partial over such a cache: the same split geometry, len_dev rule and fp32
 *   partials (part_m, part_l, part_o; the neutral element for a split without keys), which vita_decode_attn_merge and the
 *   context-parallel message take unchanged.  Scores and P.V are computed as for bf16 K / V on the codes; the K scale multiplies
 *   the finished dot product, the V scale multiplies p.
 * vita_decode_layer_attn_kv8: vita_decode_layer_attn with the cache described by `c`; k_cache, v_cache, kv_row_stride and
 *   kv_group_stride of the parameter struct are not read.  The appended row holds the codes and scales of the rule applied to the
 *   K / V row vita_decode_layer_attn appends; the context is that of vita_kv8_store + vita_decode_attn_partial_kv8 +
 *   vita_decode_attn_merge, bit for bit.  vita_decode_layer_mlp follows unchanged.
 * vita_kv8_load: the mirror of vita_kv8_store: reads rows [0, rows) of such a cache back as bf16 into k_dst / v_dst (row 0, group 0;
 *   strides in bf16 elements, multiples of 8, pointers 16-byte aligned): x~_i = bf16_rne(f32(code_i) * s), one fp32 multiply and one
 *   round-to-nearest-even conversion; non-finite stays non-finite.  Nothing outside those rows is read or written, the padding
 *   between rows and groups included.  A cached call of q_len > 1 tokens behind an FP8 cache stages the earlier rows this way and
 *   runs vita_flash_attn_extend_fwd on the staging buffer.  head_dim != 128, misaligned pointers or strides, rows * groups > 2^40:
 *   VITA_ERR_UNSUPPORTED; a null pointer, rows <= 0 or groups <= 0: VITA_ERR_INVALID_ARG; nothing is launched.
 * Stands behind Megatron's InferenceParams.key_value_memory_dict (Attention._adjust_key_value_for_inference under the decode loop
 * M/inference/text_generation/generation.py:127-131) and the HF cache update of modeling_long_vita.py:150-202. */
typedef struct {
  void *k_codes, *v_codes;       /* [capacity][kv_groups][128] e4m3fn */
  int64_t code_row_stride, code_group_stride;   /* bytes */
  void *k_scales, *v_scales;     /* [capacity][kv_groups] fp32 */
  int64_t scale_row_stride, scale_group_stride; /* floats */
} vita_kv8_cache;
/* InferenceParams.key_value_memory_dict (Megatron); modeling_long_vita.py:150-202 (HF cache) */
int vita_kv8_store(const void* k_src, const void* v_src, int64_t src_row_stride, int64_t src_group_stride, int64_t rows,
                   int groups, int head_dim, void* k_codes, void* v_codes, int64_t code_row_stride, int64_t code_group_stride,
                   void* k_scales, void* v_scales, int64_t scale_row_stride, int64_t scale_group_stride, int64_t row0,
                   const void* row0_dev, int64_t capacity, void* stream);
/* the HF cache update modeling_long_vita.py:150-202 with q_len > 1 */
int vita_kv8_load(const void* k_codes, const void* v_codes, int64_t code_row_stride, int64_t code_group_stride,
                  const void* k_scales, const void* v_scales, int64_t scale_row_stride, int64_t scale_group_stride, int64_t rows,
                  int groups, int head_dim, void* k_dst, void* v_dst, int64_t dst_row_stride, int64_t dst_group_stride,
                  void* stream);
/* InferenceParams.key_value_memory_dict (Megatron); modeling_long_vita.py:150-202 (HF cache) */
int vita_decode_attn_partial_kv8(const void* q, int64_t q_group_stride, int64_t q_head_stride, const void* k_codes,
                                 const void* v_codes, int64_t code_row_stride, int64_t code_group_stride, const void* k_scales,
                                 const void* v_scales, int64_t scale_row_stride, int64_t scale_group_stride, int len,
                                 const void* len_dev, int n_splits, int groups, int qpg, int head_dim, float softmax_scale,
                                 void* part_m, void* part_l, void* part_o, void* stream);
/* InferenceParams.key_value_memory_dict (Megatron); modeling_long_vita.py:150-202 (HF cache) */
int vita_decode_layer_attn_kv8(const vita_decode_layer_params* p, const vita_kv8_cache* c, void* stream);

/* ---------------------------------------------------------------------------------------------
 * FP8 decoder weights for the cached token step (opt-in, CP = 1 and TP = 1).  The four linears of a decoder layer
 * (linear_qkv, linear_proj, linear_fc1, linear_fc2) are kept a second time as OCP e4m3fn codes [N][K] (1 byte per element, row
 * stride in BYTES, a multiple of 16, pointer 16-byte aligned) plus one fp32 scale per run of 128 consecutive K elements of a row,
 * scales [N][K / 128] dense: 0.516 of the bf16 bytes.  The rule is the KV cache's, per run w[0..127]: amax = max |w_i|;
 * s = amax > 0 ? amax / 448 : 1; code_i = e4m3fn_rne(w_i / s) (fp32, IEEE division, no clamp); the GEMV computes with
 * f32(code_i) * s.  K must be a multiple of 128 (else VITA_ERR_UNSUPPORTED, as for misaligned codes or scales).
 *
 * vita_w8_quantize: W [N][K] bf16 (row stride ldw in elements, a multiple of 8, pointer 16-byte aligned) -> codes and scales.
 *   Bytes of a code row behind K are not written.  Runs once per weight.
 * vita_gemv_w8: vita_gemv_bf16 over codes and scales: y[N] = epilogue(dequant(codes, scales)[N,K] . x[K]), the epilogues NONE /
 *   BIAS / RESIDUAL / SWIGLU (codes and scales of cat[gate, up], 2 N rows) with vita_gemv_bf16's rounding chain; gamma != NULL:
 *   x is RMS-normalised first (gamma [K], eps) with the arithmetic the fused layer entries use on the bf16 path.  The products are
 *   summed in fp32, a run's scale multiplies a lane's finished partial sum, nothing is rounded to bf16 in front of the epilogue.
 *   Rows behind N and columns behind K are never read.
 * vita_gemv_rows_w8: vita_gemv_w8 for the rows x[b][K], b < rows <= 8, of the multi-row decode steps (x, y, R through their row
 *   strides ldx, ldy, ldr in elements, as vita_gemv_rows_bf16): y[b][N] = epilogue(dequant(codes, scales)[N,K] . x[b][K]).  Every code
 *   row and its scales are read once for all input rows, and row b has the bits of vita_gemv_w8 (gamma = NULL) on row b.  No folded
 *   RMSNorm: the caller normalises the rows once with vita_rmsnorm_fwd.  RESIDUAL: y may alias R.  rows > 8, K % 128 != 0,
 *   ldx % 8 != 0, ldx < K, ldy < N, ldc_bytes % 16 != 0 or < K, misaligned x / codes / scales: VITA_ERR_UNSUPPORTED.  Nothing behind
 *   code row N (2 N for SWIGLU), column K or input row rows - 1 is read.
 * vita_decode_layer_attn_w8 / vita_decode_layer_mlp_w8: vita_decode_layer_attn / _mlp with the four GEMVs of the layer reading
 *   the codes and scales of `w` (dense: row stride K); qkv_w, o_w, fc1_w and fc2_w of the parameter struct are not read.
 *   kv8 != NULL: the cache is the FP8 cache it describes, as for vita_decode_layer_attn_kv8; NULL: the bf16 cache of the
 *   parameter struct.  The same kernels as vita_gemv_w8 and the separate attention entries, bit for bit.  hidden and ffn must be
 *   multiples of 128.
 * Stand behind the linears of M/core/tensor_parallel/layers.py:825 at sq = 1, under the decode loop
 * M/inference/text_generation/generation.py:127-131. */
typedef struct {
  const void *qkv_codes, *o_codes, *fc1_codes, *fc2_codes;      /* e4m3fn [N][K], dense, 16-byte aligned */
  const void *qkv_scales, *o_scales, *fc1_scales, *fc2_scales;  /* fp32 [N][K / 128], dense */
} vita_w8_layer;
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_w8_quantize(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ldc_bytes, void* scales, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_gemv_w8(const void* x, const void* codes, int64_t ldc_bytes, const void* scales, void* y, int64_t N, int64_t K,
                 int epilogue, const void* bias, const void* R, const void* gamma, float eps, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 for up to 8 rows (beam search M/inference/text_generation/generation.py:283-471,
 * the batch_size > 1 decode loop :33-280) */
int vita_gemv_rows_w8(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc_bytes, const void* scales, void* y,
                      int64_t ldy, int64_t N, int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_decode_layer_attn_w8(const vita_decode_layer_params* p, const vita_w8_layer* w, const vita_kv8_cache* kv8, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_decode_layer_mlp_w8(const vita_decode_layer_params* p, const vita_w8_layer* w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MXFP4 decoder weights for the cached token step (opt-in, CP = 1 and TP = 1): the third value of the switch the
 * FP8 weights above are the second of, with the same life cycle.  The four linears of a decoder layer are kept a second time as
 * OCP e2m1 codes [N][K / 2] (two codes per byte: byte j of a row holds element 2 j in bits 0-3 and element 2 j + 1 in bits 4-7; row
 * stride in BYTES, a multiple of 16, pointer 16-byte aligned) plus one E8M0 scale byte per run of 32 consecutive K elements of a
 * row, scales [N][K / 32] dense: 0.266 of the bf16 bytes.  The rule (csrc/mx4_rule.h), per run w[0..31]: amax = max |w_i|;
 * amax == 0: e = 0, else e = the smallest integer with amax <= 6 * 2^e, clamped to [-126, 127]; scale byte = e + 127;
 * code_i = sign << 3 | idx with idx the index in {0, 0.5, 1, 1.5, 2, 3, 4, 6} nearest to |w_i| / 2^e, ties to the even index, the
 * sign kept also on a zero; nothing is clamped.  A run with a non-finite element gets scale byte 0xFF and codes 0; the GEMVs read a
 * scale byte as the float (byte << 23), so such a run makes its outputs non-finite.  The GEMV computes with
 * grid[idx] * (+-1) * 2^e.  K must be a multiple of 32 (else VITA_ERR_UNSUPPORTED, as for a misaligned code base or stride).
 *
 * vita_mx4_quantize: W [N][K] bf16 (row stride ldw in elements, a multiple of 8, pointer 16-byte aligned) -> codes and scales.
 *   Bytes of a code row behind K / 2 are not written.  Runs once per weight.
 * vita_gemv_mx4: vita_gemv_w8 over these codes and scales, the same epilogues (SWIGLU: codes and scales of cat[gate, up], 2 N
 *   rows) and the same folded RMSNorm (gamma != NULL).  The products are summed in fp32, a run's scale multiplies a lane's
 *   finished 16-element partial sum, nothing is rounded to bf16 in front of the epilogue.  Rows behind N and columns behind K are
 *   never read.
 * vita_gemv_rows_mx4: vita_gemv_mx4 for the rows x[b][K], b < rows, 1 <= rows <= 8 (else VITA_ERR_UNSUPPORTED), of the multi-row
 *   decode steps (x, y, R through their row strides ldx, ldy, ldr in elements): every code row and its scales are read once for all
 *   input rows, and row b has the bits of vita_gemv_mx4 (gamma = NULL) on row b.  No folded RMSNorm.  RESIDUAL: y may alias R.
 *   Nothing behind code row N (2 N for SWIGLU), column K or input row rows - 1 is read.
 * vita_decode_layer_attn_mx4 / vita_decode_layer_mlp_mx4: vita_decode_layer_attn_w8 / _mlp_w8 with the four GEMVs reading the codes
 *   and scales of `w` (dense: row stride K / 2); kv8 as there.  hidden and ffn must be multiples of 32.
 * Stand behind the linears of M/core/tensor_parallel/layers.py:825 at sq = 1, under the decode loop
 * M/inference/text_generation/generation.py:127-131. */
typedef struct {
  const void *qkv_codes, *o_codes, *fc1_codes, *fc2_codes;      /* e2m1 pairs [N][K / 2], dense, 16-byte aligned */
  const void *qkv_scales, *o_scales, *fc1_scales, *fc2_scales;  /* E8M0 bytes [N][K / 32], dense */
} vita_mx4_layer;
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_mx4_quantize(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ldc_bytes, void* scales, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_gemv_mx4(const void* x, const void* codes, int64_t ldc_bytes, const void* scales, void* y, int64_t N, int64_t K,
                  int epilogue, const void* bias, const void* R, const void* gamma, float eps, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 for up to 8 rows (beam search M/inference/text_generation/generation.py:283-471,
 * the batch_size > 1 decode loop :33-280) */
int vita_gemv_rows_mx4(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc_bytes, const void* scales, void* y,
                       int64_t ldy, int64_t N, int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_decode_layer_attn_mx4(const vita_decode_layer_params* p, const vita_mx4_layer* w, const vita_kv8_cache* kv8, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq = 1 (decode loop M/inference/text_generation/generation.py:127-131) */
int vita_decode_layer_mlp_mx4(const vita_decode_layer_params* p, const vita_mx4_layer* w, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MXFP8 for the prefill GEMMs (opt-in, CP = 1 and TP = 1): the four linears of a decoder layer on the block-scaled
 * matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4, which runs e4m3 operands at twice the bf16 rate and applies one E8M0 scale
 * per 32 K elements in hardware.  Both operands are quantised: the weights once (kept beside the bf16 weights, 0.516 of their bytes),
 * the activation rows of every linear in a pass of their own.  A matrix [rows][K] is kept as OCP e4m3fn codes [rows][K], one byte
 * each (row stride in BYTES, a multiple of 16, pointer 16-byte aligned), plus one E8M0 scale byte per run of 32 consecutive K
 * elements of a row, scales [rows][K / 32] dense.  The rule (csrc/mx8_rule.h), per run x[0..31]: amax = max |x_i|; amax == 0:
 * e = 0, else e = the smallest integer with amax <= 448 * 2^e, clamped to [-126, 127]; scale byte = e + 127;
 * code_i = e4m3fn_rne(x_i / 2^e), the sign kept also on a zero; nothing is clamped.  A run with a non-finite element gets scale byte
 * 0xFF and codes 0x7F (NaN): either alone makes the instruction's result NaN, so every output that reads the run is NaN.  The GEMM
 * computes with f32(code_i) * 2^e.
 *
 * vita_mx8_quantize: X [rows][K] bf16 (row stride ldx in elements, a multiple of 8, pointer 16-byte aligned) -> codes and scales.
 *   K a multiple of 32 (else VITA_ERR_UNSUPPORTED, as for a misaligned base or stride, ldx < K or ldc_bytes < K).  Bytes of a code
 *   row behind K are not written, rows behind `rows` are not touched.  A null pointer, rows <= 0 or K <= 0: VITA_ERR_INVALID_ARG.
 * vita_gemm_mx8: C[M][N] bf16 = epilogue(sum_k dequant(A)[m][k] * dequant(W)[n][k]), fp32 accumulators (inside one instruction the
 *   128 products are summed by the hardware; between instructions in fp32, ascending k).  Epilogues VITA_EPI_NONE, _BIAS, _RESIDUAL
 *   (bias may be NULL) and _SWIGLU (W holds [gate(N) ; up(N)] = 2 N rows) with exactly vita_gemm_bf16's rounding order; any other
 *   value, a missing bias (_BIAS) or R (_RESIDUAL), a null pointer, M, N or K <= 0: VITA_ERR_INVALID_ARG.  C may alias R.  Any
 *   M >= 1: rows behind M are neither read nor written.  K and N multiples of 128, else VITA_ERR_UNSUPPORTED, as are: code bases not
 *   16-byte aligned or code strides not multiples of 16 or < K; scale bases not 4-byte aligned; C / R / bias not 8-byte aligned, ldc
 *   or ldr not a multiple of 4 or < N; M or K >= 2^31, N >= 2^30.  Nothing is launched on a refusal.  A row's bits do not depend on
 *   M or on the tile the row falls in: every output element is one chain of K / 128 instructions in ascending k.
 * Stand behind the linears of M/core/tensor_parallel/layers.py:825 in the prefill (M/core/models/multimodal/gpt_vl_model.py:339-347). */
/* the input rows of the linears of M/core/tensor_parallel/layers.py:825 and their weights, quantised for vita_gemm_mx8 */
int vita_mx8_quantize(const void* X, int64_t ldx, int64_t rows, int64_t K, void* codes, int64_t ldc_bytes, void* scales, void* stream);
/* the linears of M/core/tensor_parallel/layers.py:825 at sq > 1 (prefill, M/core/models/multimodal/gpt_vl_model.py:339-347) */
int vita_gemm_mx8(const void* A_codes, int64_t lda_bytes, const void* A_scales, const void* W_codes, int64_t ldw_bytes,
                  const void* W_scales, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue, const void* bias,
                  const void* R, int64_t ldr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame / image preprocessing — ImageProcessor.process_images and dynamic_preprocess,
 * H/data/processor/image_processor.py:180-223,404-448, then the bf16 cast of
 * M/tasks/inference/module.py:693.  frames [n][height][width][3] uint8 RGB (frame_stride bytes apart)
 *   -> pad_to_square != 0: expand2square with pad_rgb (:189-201)
 *   -> Pillow BICUBIC resize to out_w x out_h (:206-208 / :429, :443; 22-bit fixed-point separable passes with a
 *      uint8 intermediate, bit-exact)
 *   -> optionally pasted at (off_x, off_y) onto a canvas_w x canvas_h canvas (resize_and_pad_image :322-362; the caller
 *      pre-fills `images` with the normalised pad colour; canvas_w <= 0: no canvas)
 *   -> cut into tile x tile blocks in row-major order (the crop loops :431-441, :365-384; tile == out_w == out_h: one block)
 *   -> (x * 1.0 / 255.0 - mean) / std in float32 (:210-215) -> images [n * blocks][3][tile][tile] bf16.
 * h_bounds [out_w][2] / h_coeffs [out_w][h_ksize] and v_bounds [out_h][2] / v_coeffs [out_h][v_ksize] (int32,
 * device) are Pillow's precompute_coeffs / normalize_coeffs_8bpc tables for the (padded) source width -> out_w
 * and height -> out_h; pad_rgb, mean, std_ are HOST arrays of 3.
 * tmp: device scratch of n * source_height * out_w * 3 bytes; u8_out (optional): the uint8 resize result
 * [n][out_h][out_w][3]. */
int vita_frames_resize_norm(const void* frames, int64_t frame_stride, int n, int height, int width,
                            int pad_to_square, const int* pad_rgb, int out_w, int out_h, int tile,
                            int canvas_w, int canvas_h, int off_x, int off_y, const void* h_bounds, const void* h_coeffs, int h_ksize, const void* v_bounds,
                            const void* v_coeffs, int v_ksize, const float* mean, const float* std_,
                            void* tmp, void* images, void* u8_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VITA_HIP_H */
