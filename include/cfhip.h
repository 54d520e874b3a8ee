/*
 * cfhip.h — C-ABI of libcfhip.so: the MI355X (gfx950 / CDNA4) kernels behind carefree-learn's
 * data-parallel training hot path (ViT building blocks).
 *
 * The reference (carefree-learn v0.5.0, /root/reference) is 100 % Python and has no FFI of its
 * own: all arithmetic on this path is delegated to PyTorch ATen ops.  The "reference interface"
 * each entry point replaces is therefore the ATen call site inside the reference module, cited
 * per function below as file:line relative to /root/reference.
 *
 * Conventions
 *   - plain C types only; every tensor is a raw device pointer + explicit sizes / leading dims
 *     (in ELEMENTS of the tensor's dtype); row-major, last dimension contiguous.
 *   - bf16 = 16-bit brain float stored as uint16_t; "f32" = IEEE float.
 *   - every call takes the HIP stream (hipStream_t as void*); nothing synchronises the device,
 *     nothing allocates or frees device memory, no pointer is retained after return: the caller
 *     (PyTorch caching allocator) owns every buffer, scratch is passed in as `workspace`.
 *   - return 0 on success, negative on error; cfhip_last_error() gives the thread-local message.
 *   - re-entrant: callable from the Python main thread and the autograd worker thread.
 */
#ifndef CFHIP_H
#define CFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFHIP_VERSION 100 /* 0.1.0 */

/* error codes */
#define CFHIP_OK 0
#define CFHIP_ERR_INVALID (-1)   /* bad argument / unsupported shape */
#define CFHIP_ERR_LAUNCH (-2)    /* HIP launch failure */
#define CFHIP_ERR_WORKSPACE (-3) /* workspace too small */

int cfhip_version(void);
const char* cfhip_last_error(void);
/* tuning knobs (process-wide, used by the benchmarks' A/B runs; defaults are the shipped behaviour):
 *   "gemm_config"     -1 (shape heuristic, default) or 0..16 to force one tile configuration
 *                     (0: 128x128x64, 1: 128x128x32, 3: 128x64x64, 7: 256x256x32 two-group kernel,
 *                      8: 256x128x32 two-group kernel, 13: 256x256x64, 14 / 15: 192x128x64 on eight / four waves, 16: 128x256x64;
 *                      see csrc/gemm.hip)
 *   "gemm_heuristic"  1..8, which shape -> configuration table pick_config() uses (default 8: every M >= 1024 forward and
 *                     dX GEMM on 192x128x64 — four waves for outputs up to 1 024 columns wide, eight otherwise —, single dW GEMMs
 *                     on 128x128x32; 7: eight waves everywhere; 6: the round-2 table — forward on the BK = 64 configurations, dX on
 *                     the 256x128x32 two-group kernel)
 *   "gemm_group_n"    tile walk order of a GEMM launch: n > 0 (default 8): outputs wider than n tile columns are walked in
 *                     groups of n columns, all rows of a group first (an XCD's resident workgroups then share n B panels
 *                     that stay in its L2); n < 0: row groups of -n panels, columns outer; 0: rows outer, every column inner
 *   "ln_bwd_fused"    1 (default): cfhip_layernorm_bwd asked for dx AND dgamma / dbeta runs the one-launch kernel
 *                     (D a multiple of 8 up to 1280; round 5: not only multiples of 256); 2: only for D a multiple of 256
 *                     (rounds 3-4); 0: the round-1 one-wave-per-row kernel
 *   "gemm_cfg_nt_wide" / "gemm_cfg_nt" / "gemm_cfg_nn" / "gemm_cfg_tn"   tile configuration of one class of M >= 1024 GEMMs
 *                     (forward with N >= 2560, other forward, dX, dW); -1 (default): the heuristic table
 *   "attn_persistent" bits: 1 dK / dV pass, 2 dQ pass, 4 forward of the head_dim-64 kernels run as persistent 16-wave
 *                     workgroups (one per CU walking (batch, head) pairs, the next head's operands streaming into a second
 *                     LDS buffer) when no mask / not causal and 128 < T <= 256 — the ViT shape; default 7; 0: one workgroup
 *                     per head.  Results are bit-identical either way.
 *   "attn_pers_ctas"  workgroups of a persistent attention launch (default 256 = one per CU; measured in the ViT step:
 *                     128 / 192 / 224 / 256 / 512 -> 17.80 / 17.71 / 17.59 / 17.60 / 17.78 ms)
 *   "grouped_variant" ring of cfhip_gemm_bf16_grouped_tn: 0 (default) 5 slots, DMA 3 K-steps ahead; 1: 4 slots, 2 ahead;
 *                     2: 5 slots, 2 ahead; 3 / 4: DMA placement variants of 0.  +16: bias gradients reduced by the first tile
 *                     column alone instead of shared by the tile row; +32: row-major tile order (both: A/B runs);
 *   "attn_two_tiles"  bits (default 511) selecting the long-sequence attention forms (csrc/attn.hip): 1 forward, 2 dQ pass (4: also head_dim
 *                     > 48), 8 dK / dV pass of head_dim <= 64 on the two-tiles-per-wave kernels; 16: forward row sums through a ones column
 *                     when head_dim = 8 mod 16; 32: dK / dV pass of head_dim 72 .. 96 on the two-tile kernel; 64 (round 6): the plain
 *                     head_dim <= 48 dQ pass with S / dP on 32x32x16 MFMAs; 128 (round 6): head_dim 40, plain: dP - delta out of the matrix
 *                     pipe (two spare reduction columns) in the dQ and dK / dV passes; 256 (round 6): head_dim 72 .. 96 without a mask: forward and dQ
 *                     pass on the two-tile kernels.  "attn_one_pass" (default 2; 0 = two passes, 1 = the 16-wave
 *                     kernel at every length, 2 = 128 < T <= 224 on 8 waves with two key tiles each, bit-identical): dQ, dK, dV of a short
 *                     self-attention from one evaluation of S and dP.  "attn_short_max": longest head_dim-64 sequence on the LDS-resident kernels
 *   "conv_form"       tile form of cfhip_conv3x3_nhwc_bf16: -1 (default) = by shape (128x160x64 on four waves where 160-column tiles cover
 *                     Cout with at most 1/8 of waste — the UNet's 320 / 640 / 960 / 1280 / 1920 / 2560 — and Cin % 64 == 0; otherwise
 *                     the round-3 table); -2: the round-3 table everywhere; 0: 256x128x32 two-group kernel, 1: 128x128x32, 2: 128x160x32, 3: 128x160x64
 *   "conv_split"      -1 (default): the K split cfhip_conv3x3_workspace sizes for; n >= 1 forces n (A/B runs; size the workspace
 *                     with the option already set)
 * Unknown names are an error.  (The phase-timing ablation masks "gemm_ablate" / "attn_ablate" of round 1 are
 * not part of this library any more: they exist only in the -DCFHIP_ABLATE build that tools/build_variant.sh
 * writes to tools/libcfhip_ablate.so, selected by the tools through CFHIP_LIB.) */
int cfhip_set_option(const char* name, int value);

/* ------------------------------------------------------------------------------------------
 * K1/K2  GEMM  (replaces F.linear at modules/core/customs.py:89, attentions.py:214,
 *              nn.Linear.forward via hijacks.py:42-57, and its autograd backward)
 *
 *   C[m][n] = epilogue( sum_k A(m,k) * B(n,k) )          bf16 operands, fp32 accumulate (MFMA)
 *
 *   a_trans = 0: A(m,k) = A[m*lda + k]      a_trans = 1: A(m,k) = A[k*lda + m]
 *   b_trans = 0: B(n,k) = B[n*ldb + k]      b_trans = 1: B(n,k) = B[k*ldb + n]
 *   (forward  y = x W^T      : a_trans 0, b_trans 0, A = x [M,K],  B = W  [N,K])
 *   (backward dx = dy W      : a_trans 0, b_trans 1, A = dy [M,Kd], B = W  [Kd,N])
 *   (backward dW = dy^T x    : a_trans 1, b_trans 1, A = dy [Kd,M], B = x  [Kd,N])
 *
 *   epilogue (bias is fp32 [N] or NULL in every mode):
 *     CFHIP_EPI_NONE        C = acc + bias
 *     CFHIP_EPI_GELU        aux_out (bf16 [M,ldc], may be NULL) = acc + bias ; C = gelu_erf(acc + bias)
 *     CFHIP_EPI_RESIDUAL    C = acc + bias + aux_in (bf16 [M,ldc]; f32 when out_dtype == 1)
 *     CFHIP_EPI_DGELU       C = acc * gelu_erf'(aux_in)   (aux_in = saved pre-activation, bf16)
 *     CFHIP_EPI_QGELU / CFHIP_EPI_DQGELU   the same two with quick GELU x * sigmoid(1.702 x)
 *                           (activations.py "quick_gelu": the CLIP towers, multimodal/clip.py)
 *   out_dtype: 0 = bf16, 1 = f32.   accumulate != 0 (f32 output only): C += result.
 *   split_k > 1: the K range is cut in `split_k` slices, partial tiles go to `workspace`
 *     (needs split_k*M*N*4 bytes) and a second kernel reduces them (epilogue NONE only).
 *   bias_grad (layout (1,1) only, else NULL): f32 [M], (+)= sum_k A(m,k) — for dW = dY^T X this is
 *     the bias gradient colsum(dY), produced by the same kernel with a ones-operand MFMA
 *     (workspace then needs split_k*M*4 more bytes).
 * ------------------------------------------------------------------------------------------ */
#define CFHIP_EPI_NONE 0
#define CFHIP_EPI_GELU 1
#define CFHIP_EPI_RESIDUAL 2
#define CFHIP_EPI_DGELU 3
#define CFHIP_EPI_QGELU 4
#define CFHIP_EPI_DQGELU 5

int cfhip_gemm_bf16(const void* A, const void* B, void* C, const float* bias, const void* aux_in,
                    void* aux_out, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                    int a_trans, int b_trans, int epilogue, int out_dtype, int accumulate,
                    int split_k, void* workspace, size_t workspace_bytes, float* bias_grad,
                    int bias_grad_accumulate, void* stream);

/* The kernel instantiation (as a profiler prints it, e.g. "gemm_bf16_kernel<false, true, 0, Cfg<192, 128, 2, 2, 2, 64>>") that
 * cfhip_gemm_bf16 launches for an aligned problem of this shape under the current options; `out` holds at least 96 bytes.
 * For evidence lines (bench.py groups its in-step timings by it); not needed to run anything. */
int cfhip_gemm_kernel_name(int M, int N, int K, int a_trans, int b_trans, int epilogue, char* out, size_t out_bytes);

/* The tile configuration (a value of the "gemm_config" option, reroutes applied) on which the calling thread's latest
 * cfhip_gemm_bf16 / cfhip_gemm_bf16_rows request was launched; -1: the generic kernel; -2: no request yet.  Host only, for tests:
 * cfhip_gemm_kernel_name answers for a shape, this for the launch that was made (cfhip_gemm_bf16_rows: under `config_rows`). */
int cfhip_gemm_last_config(void);

/* Grouped weight gradients: dW_i[M_i][N_i] (+)= dY_i^T X_i and db_i[M_i] (+)= colsum(dY_i) for `count` Linear layers in ONE
 * launch (the parameter half of F.linear's autograd backward, customs.py:89 / attentions.py:214: grad_weight =
 * grad_output^T @ input, grad_bias = grad_output.sum(0), for every Linear of one or more blocks).  Layout (1,1) of
 * cfhip_gemm_bf16: A = dY [K][M] (lda), B = X [K][N] (ldb), both bf16 token-major; C f32 [M][N] (ldc).  256 x 256 output
 * tiles of all problems share the chip, every tile runs its whole reduction: no split-K, no workspace, no second pass,
 * deterministic.  M, N, lda, ldb multiples of 8, ldc of 4, 16-byte aligned bases, K*ld*2 < 2 GiB.  `problems` is a HOST
 * array (copied into the kernel arguments, 24 per launch).  Every problem of the table is checked before the first launch: a
 * table with an invalid problem (CFHIP_ERR_INVALID, the message names its index) launches nothing and writes nothing, however
 * many launches it would have been cut into.  bias_grad may be NULL per problem.  With bias gradients the
 * workgroups of a tile row share the column-sum reduction and meet in a small workspace the LIBRARY owns, one per stream
 * (<= 16 streams; allocated on the first such launch of a stream — before any hipGraph capture); partial sums are added in a
 * fixed order, results do not depend on arrival order. */
typedef struct cfhip_gemm_problem {
  const void* A;
  const void* B;
  void* C;
  float* bias_grad;
  int M, N, K;
  /* Row period of A.  0: dense.  p > 0: the CALLER GUARANTEES that every row r of A with r % p != 0 is zero (the head-token
   * rows of a [batch * tokens] gradient: p = tokens); a tile then walks only the ceil(K / p) 32-row K-steps that hold a row
   * r = t * p instead of all ceil(K / 32), and C and bias_grad are bit-identical to the dense launch (the skipped steps
   * add products with a zero row of A; rows of B in them are not read).  p must be at least 32, the depth of a K-step:
   * 0 < p < 32 is rejected (pass 0).  A launch may mix dense and periodic problems.
   * The newest field; it occupies the four bytes that used to pad `K` up to the 8-byte `lda`, so the size of the struct (80) and
   * the offset of every other field are what they were.  A zero-initialised struct is a dense problem. */
  int k_period;
  int64_t lda, ldb, ldc;
  int accumulate;            /* C += */
  int bias_grad_accumulate;  /* bias_grad += */
} cfhip_gemm_problem;
int cfhip_gemm_bf16_grouped_tn(const cfhip_gemm_problem* problems, int count, void* stream);

/* column sums of a bf16 matrix: out[n] (f32) (+)= sum_m X[m*ldx + n]   (bias gradients)
 * workspace: >= cfhip_colsum_workspace(M, N) bytes. */
size_t cfhip_colsum_workspace(int M, int N);
int cfhip_colsum_bf16(const void* X, float* out, int M, int N, int64_t ldx, int accumulate,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K5  LayerNorm over the last dim (replaces nn.LayerNorm built by NormFactory("layer"),
 *     modules/core/norms.py:88-89,118-119; call sites mixed_stacks/api.py:141,155,397-402)
 *   biased variance, eps inside the sqrt, fp32 statistics; gamma / beta fp32; dtype_flags bit 0: x is f32 (else bf16) —
 *   the residual stream is kept in f32, as it is in the reference's autocast run (head_token / pos_encoding are f32
 *   parameters, so `x + f(LN(x))` type-promotes to f32); bit 1: y is f32 (else bf16; f32 rows only) — a LayerNorm whose
 *   output IS the residual stream (the `embedding_norm` in front of CLIP's vision blocks, cv/encoder/transformer.py:60-64:
 *   nn.LayerNorm on an f32 input returns f32 under autocast; round 6, found by the full-size CLIP parity test).
 *   D % 4 == 0 and D <= 2048 (a row lives in the registers of one wave).
 *   x_row_stride / y_row_stride in elements (lets the head LN read token 0 of every sample).
 *   fwd saves mean / rstd (f32 [M]) for bwd.
 *   bwd: dx (bf16) = LN'(dy) [+ dx_add (bf16) if not NULL]; dgamma / dbeta (f32 [D]) (+)= ...
 *        workspace >= cfhip_layernorm_bwd_workspace(M, D) bytes.  dx == NULL: parameter gradients
 *        only; dgamma == dbeta == NULL: input gradient only (two launches that can run on two
 *        streams: dx is the critical path of backward, the parameter gradients are not).
 * ------------------------------------------------------------------------------------------ */
int cfhip_layernorm_fwd(const void* x, int dtype_flags, const float* gamma, const float* beta, void* y,
                        float* mean, float* rstd, int M, int D, int64_t x_row_stride,
                        int64_t y_row_stride, float eps, void* stream);
size_t cfhip_layernorm_bwd_workspace(int M, int D);
int cfhip_layernorm_bwd(const void* dy, const void* x, int x_is_f32, const float* gamma, const float* mean,
                        const float* rstd, const void* dx_add, void* dx, float* dgamma, float* dbeta,
                        int M, int D, int64_t dy_row_stride, int64_t x_row_stride,
                        int64_t dx_row_stride, int accumulate_param_grads, void* workspace,
                        size_t workspace_bytes, void* stream);
/* cfhip_layernorm_bwd in two calls: `_partials` = the row kernel (dx (+ dx_add), per-workgroup partial sums of dgamma | dbeta into
 * `workspace`, *rows_out = number of partial rows), `_reduce` = their column sums (+)= into dgamma / dbeta on any stream the caller
 * orders behind it.  The input gradient is on the backward's critical chain, the parameter gradients are not. */
int cfhip_layernorm_bwd_partials(const void* dy, const void* x, int x_is_f32, const float* gamma, const float* mean,
                                 const float* rstd, const void* dx_add, void* dx, int M, int D, int64_t dy_row_stride,
                                 int64_t x_row_stride, int64_t dx_row_stride, void* workspace, size_t workspace_bytes,
                                 int* rows_out, void* stream);
int cfhip_layernorm_bwd_reduce(void* workspace, int rows, int D, float* dgamma, float* dbeta, int accumulate, void* stream);
/* cfhip_layernorm_bwd / _partials with the residual-gradient stream carried in TWO bf16 words per element (round 6): hi = bf16(g),
 * lo = bf16(g - hi), i.e. 16 mantissa bits.  The reference's residual stream is f32 under autocast (x + f(LN(x)) with f32 x), so the
 * gradient that flows along it is f32 and only the matrix products see it rounded to bf16; with one bf16 word the running sum is
 * rounded twice per block, and parameters whose per-sample gradients cancel (CLIP's head token / positional encoding under the
 * contrastive loss) came out 1.5 x further from fp32 than the reference's own bf16 run.  dx_add_lo / dx_lo: the second words of
 * dx_add / dx (same strides; either may be NULL); the GEMMs of the block keep reading the first word = bf16(g), as the reference's
 * do.  rows_out != NULL selects the `_partials` form (row kernel only; reduce with cfhip_layernorm_bwd_reduce). */
int cfhip_layernorm_bwd2(const void* dy, const void* x, int x_is_f32, const float* gamma, const float* mean,
                         const float* rstd, const void* dx_add, const void* dx_add_lo, void* dx, void* dx_lo,
                         float* dgamma, float* dbeta, int M, int D, int64_t dy_row_stride, int64_t x_row_stride,
                         int64_t dx_row_stride, int accumulate_param_grads, void* workspace, size_t workspace_bytes,
                         int* rows_out, void* stream);
/* The reference's 4-D `LN` (modules/core/norms.py:30-46: NormFactory("layer_norm") on [B, C, H, W]): y = (x - mean_b) / (std_b + eps) *
 * weight[c] + bias[c], ONE mean and one UNBIASED standard deviation per sample over all C*H*W elements, eps added to the standard
 * deviation.  x / y / dy / dx bf16 NCHW (contiguous); weight / bias f32 [C] or both NULL (elementwise_affine = False); mean / std f32 [B]
 * written by the forward, read by the backward.  dx == NULL: parameter gradients only; dweight == dbias == NULL: dx only.
 * workspace >= cfhip_layernorm4d_workspace(B, C, HW) bytes.  Fixed summation order: results are reproducible bit for bit. */
size_t cfhip_layernorm4d_workspace(int B, int C, int HW);
int cfhip_layernorm4d_fwd(const void* x, const float* weight, const float* bias, void* y, float* mean, float* std, int B, int C,
                          int HW, float eps, void* workspace, size_t workspace_bytes, void* stream);
int cfhip_layernorm4d_bwd(const void* dy, const void* x, const float* weight, const float* mean, const float* std, void* dx,
                          float* dweight, float* dbias, int accumulate_param_grads, int B, int C, int HW, float eps, void* workspace,
                          size_t workspace_bytes, void* stream);
/* the two ends of that stream: f32 -> (hi, lo) and (hi, lo) -> f32 = hi + lo (exact in f32) */
int cfhip_split_f32_bf16x2(const float* src, void* hi, void* lo, int64_t n, void* stream);
int cfhip_join_bf16x2_f32(const void* hi, const void* lo, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * K3/K4  fused scaled-dot-product attention (replaces F.scaled_dot_product_attention reached
 *     through sdp_attn, toolkit.py:953-963, from Attention.forward, attentions.py:254, and the
 *     head split / merge copies at attentions.py:180-185,270-275)
 *
 *   o[b,t,h,:] = softmax_j( q[b,t,h,:] . k[b,j,h,:] * scale  [+ mask] ) v[b,j,h,:]
 *
 *   q, k, v, o, dq, dk, dv, do: bf16, addressed as  ptr[b*stride_b + t*stride_t + h*DH + d]
 *   (so the packed [B,T,3,H,DH] projection output is consumed in place and o is written
 *   directly as [B,T,H*DH]).  head_dim DH must be 64.  Tq, Tk <= CFHIP_ATTN_MAX_T: the whole K/V of
 *   one head is LDS-resident (one workgroup per (b, h)); longer sequences: the same kernels with an
 *   outer loop over 256-row chunks (online softmax across chunks in the forward, one workgroup per
 *   128 query / key rows).  lse: f32 [B,H,Tq] (natural-log sum-exp of the scaled scores).
 *   mask: optional uint8 "keep" mask (1 = attend), addressed mask[b*ms_b + h*ms_h + i*ms_q + j]
 *   (strides may be 0 for broadcasting), or NULL.  causal != 0 additionally masks j > i.
 *   bwd needs delta: f32 [B,H,Tq] scratch (rowsum(do * o), computed inside).
 *   A query row WITHOUT ANY KEPT KEY (mask only; a causal row always keeps j = 0) has 1 / l with l = 0: that row's own
 *   o, lse and dq are unspecified (NaN or anything else).  Every other row of o / lse / dq and every row of dk / dv is
 *   what it would be without that row (it contributes exactly 0 to dk / dv, also when the o and lse handed back to the
 *   backward hold NaN there), and nothing outside the outputs is written.
 * ------------------------------------------------------------------------------------------ */
#define CFHIP_ATTN_MAX_T 256
#define CFHIP_ATTN_HEAD_DIM 64

int cfhip_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse,
                   const uint8_t* mask, int B, int H, int Tq, int Tk, int64_t q_stride_b,
                   int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t, int64_t o_stride_b,
                   int64_t o_stride_t, int64_t ms_b, int64_t ms_h, int64_t ms_q, float scale,
                   int causal, void* stream);

int cfhip_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                   const float* lse, float* delta, const uint8_t* mask, void* dq, void* dk, void* dv,
                   int B, int H, int Tq, int Tk, int64_t q_stride_b, int64_t q_stride_t,
                   int64_t kv_stride_b, int64_t kv_stride_t, int64_t o_stride_b, int64_t o_stride_t,
                   int64_t ms_b, int64_t ms_h, int64_t ms_q, float scale, int causal, int parts,
                   void* stream);
/* Attention with RETURNED weights — the reference's slow path `Attention.forward(require_weights=True)` / `customize_sdp`
 * (attentions.py:256-268: raw = q k^T / scaling, masked_fill(-inf), softmax, weights @ v).  The output comes from
 * cfhip_attn_fwd_dh with scale = 1 / scaling; cfhip_attn_probs materialises what the fused kernels never store:
 *     probs[b][h][i][j] (f32) = keep(b,h,i,j) ? exp(scale * q_i . k_j - lse[b][h][i]) : 0
 * and cfhip_attn_probs_bwd turns a gradient on those weights into its dq / dk contribution through the softmax
 *     t_i = sum_j dP_ij P_ij;  dS_ij = scale P_ij (dP_ij - t_i);  dq_i = sum_j dS_ij k_j;  dk_j = sum_i dS_ij q_i
 * (written as bf16 [B][T][H*head_dim] contiguous; the caller adds them to cfhip_attn_bwd_dh's; dv gets nothing).
 * ds_workspace: f32 [B][H][Tq][Tk].  fp32 VALU arithmetic, no atomics (deterministic); an inspection / auxiliary-loss path,
 * not a throughput path.  Addressing, mask and causal conventions as cfhip_attn_fwd_dh; head_dim a multiple of 8 up to 192. */
int cfhip_attn_probs(const void* q, const void* k, const float* lse, const uint8_t* mask, float* probs, int B, int H,
                     int Tq, int Tk, int head_dim, int64_t q_stride_b, int64_t q_stride_t, int64_t k_stride_b,
                     int64_t k_stride_t, int64_t ms_b, int64_t ms_h, int64_t ms_q, float scale, int causal, void* stream);
int cfhip_attn_probs_bwd(const void* q, const void* k, const float* lse, const uint8_t* mask, const float* d_probs,
                         float* ds_workspace, void* dq, void* dk, int B, int H, int Tq, int Tk, int head_dim,
                         int64_t q_stride_b, int64_t q_stride_t, int64_t k_stride_b, int64_t k_stride_t, int64_t ms_b,
                         int64_t ms_h, int64_t ms_q, float scale, int causal, void* stream);

/* The same with an explicit head_dim (any multiple of 8 up to 192, e.g. the 40 / 80 / 160-channel heads of the UNet's
 * SpatialTransformer, mixed_stacks/api.py:766-893; attentions.py:498-569): always the chunked general kernels unless
 * head_dim == 64 and both lengths fit the resident form.  Addressing ptr[b*stride_b + t*stride_t + h*head_dim + d]. */
int cfhip_attn_fwd_dh(const void* q, const void* k, const void* v, void* o, float* lse,
                      const uint8_t* mask, int B, int H, int Tq, int Tk, int head_dim, int64_t q_stride_b,
                      int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t, int64_t o_stride_b,
                      int64_t o_stride_t, int64_t ms_b, int64_t ms_h, int64_t ms_q, float scale, int causal,
                      void* stream);
int cfhip_attn_bwd_dh(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                      const float* lse, float* delta, const uint8_t* mask, void* dq, void* dk, void* dv,
                      int B, int H, int Tq, int Tk, int head_dim, int64_t q_stride_b, int64_t q_stride_t,
                      int64_t kv_stride_b, int64_t kv_stride_t, int64_t o_stride_b, int64_t o_stride_t,
                      int64_t ms_b, int64_t ms_h, int64_t ms_q, float scale, int causal, int parts,
                      void* stream);
/* The same with DROPOUT ON THE ATTENTION PROBABILITIES (reference attentions.py:254 -> sdp_attn(..., dropout) ->
 * F.scaled_dot_product_attention(dropout_p); attentions.py:264-265 in the weights path): O = dropout(softmax(S)) V.
 * The keep mask is a pure function of (seed, offset, b, h, i, j) — one Philox4x32-10 call per 4 x 4 block of the score
 * matrix, counter = offset + ((b H + h) ceil(Tq / 4) + i / 4) ceil(Tk / 4) + j / 4, byte (j % 4) of word (i % 4) >=
 * round(256 p) keeps — so the two backward passes regenerate it from the pair the forward used (advance `offset` by
 * B H ceil(Tq / 4) ceil(Tk / 4) per call) and no mask is ever stored.  The probability is quantised to 1/256 (kept
 * values scale by 256 / (256 - round(256 p))).  Any head_dim / length: these run the chunked kernels.
 * cfhip_attn_dropout_mask writes that mask (uint8 [B][H][Tq][Tk], 1 = keep) for tests and debugging. */
int cfhip_attn_fwd_dropout(const void* q, const void* k, const void* v, void* o, float* lse, const uint8_t* mask,
                           int B, int H, int Tq, int Tk, int head_dim, int64_t q_stride_b, int64_t q_stride_t,
                           int64_t kv_stride_b, int64_t kv_stride_t, int64_t o_stride_b, int64_t o_stride_t,
                           int64_t ms_b, int64_t ms_h, int64_t ms_q, float scale, int causal, float dropout_p,
                           uint64_t seed, uint64_t offset, void* stream);
int cfhip_attn_bwd_dropout(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                           const float* lse, float* delta, const uint8_t* mask, void* dq, void* dk, void* dv, int B,
                           int H, int Tq, int Tk, int head_dim, int64_t q_stride_b, int64_t q_stride_t,
                           int64_t kv_stride_b, int64_t kv_stride_t, int64_t o_stride_b, int64_t o_stride_t,
                           int64_t ms_b, int64_t ms_h, int64_t ms_q, float scale, int causal, int parts,
                           float dropout_p, uint64_t seed, uint64_t offset, void* stream);
int cfhip_attn_dropout_mask(void* mask_out, int B, int H, int Tq, int Tk, float dropout_p, uint64_t seed,
                            uint64_t offset, void* stream);
/* parts: 1 = dQ pass only, 2 = dK/dV pass only, 3 = both.  The two passes are independent kernels
 * (each recomputes S, dP and delta) and may be launched on two streams. */
/* The kernel instantiations a forward (backward = 0) or backward (backward != 0) call of this head_dim, these lengths and
 * this mode launches under the current options, in launch order, separated by newlines and spelled as
 * tools/attn_kernel_census.py prints a profiler's names ("attn_fwd2_kernel<true,3,true>"); `out` holds at least 128 bytes.
 * has_mask / causal / dropout: a mask is given / causal != 0 / dropout_p > 0; parts as above (ignored by the forward);
 * has_lse: the forward is given an lse buffer (ignored by the backward).  Nothing else enters the selection: no pointer,
 * no stride, no batch or head count.  A host-side query: no device is touched. */
int cfhip_attn_plan(int backward, int head_dim, int Tq, int Tk, int has_mask, int causal, int dropout, int parts,
                    int has_lse, char* out, size_t out_bytes);

/* Wide-head attention forward: ONE head as wide as the channel count — SpatialAttention (attentions.py:330-370), the
 * single-head attention over C channels at the bottleneck of the KL autoencoder (cv/ae/kl.py, cv/decoder/attn.py; C = 512 in
 * the zoo model) that the first stage of latent diffusion runs (multimodal/diffusion/ldm.py:154-202).  head_dim: any multiple
 * of 8 with 192 < head_dim <= CFHIP_ATTN_WIDE_MAX_HEAD_DIM (up to 192: cfhip_attn_fwd_dh, which keeps refusing more).
 * Operands and addressing as cfhip_attn_fwd_dh (bf16, ptr[b*stride_b + t*stride_t + h*head_dim + d], lse f32 [B][H][Tq] or
 * NULL); no mask, not causal, no dropout; forward only.  K / V stream through LDS at most CFHIP_ATTN_WIDE_CHUNK keys at a time. */
#define CFHIP_ATTN_WIDE_MAX_HEAD_DIM 512
#define CFHIP_ATTN_WIDE_CHUNK 64
int cfhip_attn_wide_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Tq, int Tk,
                        int head_dim, int64_t q_stride_b, int64_t q_stride_t, int64_t kv_stride_b, int64_t kv_stride_t,
                        int64_t o_stride_b, int64_t o_stride_t, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8 (ViT patch embedding) + K7 glue
 *   im2row: img f32/bf16 [B,C,Hh,Ww] -> rows bf16 [B*gh*gw, C*P*P] in (c, ph, pw) order, so the
 *     stride==kernel Conv2d of VanillaPatchEmbed (high_level.py:172-188) becomes one K1 GEMM with
 *     the conv weight viewed as [out, C*P*P].
 *   assemble_tokens: x0[b,0,:] = head_token + pos[0]; x0[b,1+p,:] = patches[b,p,:] + pos[1+p]
 *     (mixed_stacks/api.py:419-438,209-228).  bwd: dpatches (bf16), dhead_token, dpos (f32, (+)=).
 * ------------------------------------------------------------------------------------------ */
int cfhip_im2row(const void* img, int img_is_bf16, void* rows, int B, int C, int Hh, int Ww, int P,
                 void* stream);
int cfhip_assemble_tokens_fwd(const void* patches, const float* head_token, const float* pos,
                              void* x0, int x0_is_f32, int B, int Np, int D, void* stream);
int cfhip_assemble_tokens_bwd(const void* dx0, void* dpatches, float* dhead_token, float* dpos,
                              int B, int Np, int D, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * element-wise helpers (K6 stand-alone forms, casts)
 * ------------------------------------------------------------------------------------------ */
int cfhip_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int cfhip_cast_bf16_to_f32(const void* src, float* dst, int64_t n, void* stream);
int cfhip_gelu_fwd(const void* x, void* y, int64_t n, void* stream);              /* bf16 */
int cfhip_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, void* stream);
int cfhip_quick_gelu_fwd(const void* x, void* y, int64_t n, void* stream);        /* x * sigmoid(1.702 x) */
int cfhip_quick_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, void* stream);
/* DDPM forward process and objective (multimodal/diffusion/samplers/schema.py:90-112; models/cv/diffusion.py:44-94):
 *   q_sample: out[b][:] = sqrt_ac[t_b] * x[b][:] + sqrt_1mac[t_b] * noise[b][:]  (x, noise f32; t int64 [B]; the
 *     tables f32 [T]; f32 output bit-exact with the reference expression, or bf16)
 *   mse_loss: loss_sum (f32[1], caller zeroes) += sum_b mean_inner (pred - target)^2 ; dpred (bf16, may be NULL) =
 *     grad_scale * 2 (pred - target) / inner   (pred bf16 = the UNet output, target f32 = the noise) */
int cfhip_q_sample(const float* x, const float* noise, const int64_t* t, const float* sqrt_ac,
                   const float* sqrt_1mac, void* out, int out_is_f32, int64_t B, int64_t inner, void* stream);
int cfhip_mse_loss(const void* pred, const float* target, float* loss_sum, void* dpred, int64_t B, int64_t inner,
                   float grad_scale, void* stream);
/* DDPMStep.loss_fn (models/cv/diffusion.py:44-94) for every objective it has: per_sample[b] (f32, must be zero on entry)
 * += mean_inner f(pred - target), f = square (loss_type 0, "l2") or abs (1, "l1"); dpred (bf16, may be NULL) =
 * weight[b] * f'(pred - target) / inner.  weight f32 [B] carries everything the reference multiplies a sample's loss by
 * (l_simple_weight / exp(log_var[t]) + original_elbo_weight * lvlb_weights[t], over the batch size). */
int cfhip_diffusion_loss(const void* pred, const float* target, const float* weight, float* per_sample, void* dpred,
                         int64_t B, int64_t inner, int loss_type, void* stream);
/* Reverse diffusion (csrc/sample.hip).
 *   randn_f32: out[i] = standard normal from Philox4x32-10 at counter (seed, offset + i / 4), Box-Muller on uniforms in
 *     (0, 1], four values per counter — the starting noise z of DDPM.generate_z (multimodal/diffusion/ddpm.py:264-266).
 *   The sampler step (one kernel walk with one update rule per sampler) and its advance.  What diffusion_sample_step and
 *   k_sample_step share: x f32 [B][n] (n % 4 == 0) is the state, updated in place; out_c / out_u: bf16 model outputs [B][n],
 *     mixed by classifier-free guidance (samplers/schema.py:215-263) into m = out_u + scale (out_c - out_u) when out_u is not
 *     NULL; table: f32 [rows][row width], row k = the scalars of launch k (column 0: the UNet's timestep), formed on the host in
 *     the reference's f32 order; k: device int32 counter, and a k outside [0, rows) makes the launch a no-op; noise: f32 bank
 *     [rows][B][n], or NULL for the Philox normals of randn_f32 at counter (seed, offset + k * B n / 4 + i / 4).  Writes x and
 *     the UNet's next input xin (bf16, `dup` copies of [B][n] one after the other: 2 when guidance runs one 2B-batch forward);
 *     clip_last clamps the state the LAST row writes to [-1, 1] (DDPM.sample, ddpm.py:298-300).  The arithmetic keeps the
 *     reference's roundings (no FMA contraction, IEEE division).  Arguments outside this return -1 before any launch.
 *   diffusion_sample_step: one reverse step of DDIMSampler (samplers/ddim.py:195-239, predict_eps/start_from_z_and_v of
 *     ddpm.py:461-484; CFHIP_PARAM_EPS or _V) or BasicSampler (samplers/basic.py:61-92; CFHIP_PARAM_EPS or _X0) per row of
 *     CFHIP_SAMPLE_ROW scalars (columns per kind: csrc/sample.hip); xin = bf16(x).
 *   diffusion_sample_advance: k += 1 and timesteps[0 .. gb) = (int64) table[k][0] while k < steps; a launch of its own
 *     so that no workgroup of a step can see k change. */
#define CFHIP_SAMPLE_ROW 8
#define CFHIP_SAMPLER_DDIM 0
#define CFHIP_SAMPLER_BASIC 1
#define CFHIP_PARAM_EPS 0
#define CFHIP_PARAM_X0 1
#define CFHIP_PARAM_V 2
int cfhip_randn_f32(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream);
/* Posterior draw of the KL autoencoder, scaled into the latent a diffusion UNet trains on: GaussianDistribution (cv/ae/kl.py:
 * 18-45: chunk the moments, clamp log_var to [-30, 20], mean + exp(0.5 log_var) * randn; kl()) and LDM.preprocess's scale_factor
 * (multimodal/diffusion/ldm.py:183-190) in one launch instead of six element-wise ones:
 *     z[b][c][p] (f32, [B][E][hw] contiguous; may be NULL when only kl is wanted) =
 *         scale_factor * (mean + exp(0.5 * clamp(log_var, -30, 20)) * n)
 *   moments: bf16, [B][2E][hw] (channels_last = 0) or [B][hw][2E] (channels_last != 0) as the to_embedding convolution leaves
 *     them, read in place; mean = channels [0, E), log_var = channels [E, 2E).
 *   n: noise[b][c][p] (f32, the layout of z) when given; else, with deterministic != 0, no draw at all: z = scale_factor *
 *     mean, the mode; else the Philox stream of cfhip_randn_f32 at (seed, offset) over the flat index of z.
 *   kl (f32 [B] or NULL; overwritten, not accumulated) = 0.5 * sum_{c,p} (mean^2 + var - 1 - log_var), var = exp(clamped
 *     log_var): the KL divergence to the standard normal per sample, reduced in a fixed order. */
int cfhip_gaussian_posterior(const void* moments, int channels_last, float* z, float* kl, const float* noise, int deterministic,
                             int64_t B, int E, int64_t hw, float scale_factor, uint64_t seed, uint64_t offset, void* stream);
int cfhip_diffusion_sample_step(float* x, void* xin, const void* out_c, const void* out_u, float scale, const float* table,
                                int steps, const int* k, const float* noise, int64_t B, int64_t n, int kind, int param,
                                float temperature, int clip_last, int dup, uint64_t seed, uint64_t offset, void* stream);
int cfhip_diffusion_sample_advance(int* k, const float* table, int steps, int64_t* timesteps, int gb, void* stream);
/* The sigma-space "K" samplers (samplers/k_samplers.py): KEulerAncestralSampler (:367-397), KHeunSampler (:400-440) and
 * KDPMpp2MSampler (:443-477) around IKSampler.sample_step's get_denoised (:152-183), on the step kernel and the contract above.
 *   k_sample_step: ONE launch per model evaluation.  Row k of CFHIP_KSAMPLE_ROW scalars is EVALUATION k (k_heun has two per step):
 *       0 t (the UNet's timestep)  1 sigma  2 c_out  3 c_skip  4 c_in of the NEXT evaluation's input  5 dt  6 sigma_up
 *       7 sigma_next / sigma  8 expm1(-h)  9 1 + 1 / (2 r)  10 1 / (2 r)
 *       11 flag: euler_a next_sigma > 0 (add the draw); heun 0 = stage 1, 1 = stage 2; dpmpp_2m 1 = old_denoised exists.
 *     denoised = img - m c_out (CFHIP_PARAM_EPS) or img c_skip - m c_out (CFHIP_PARAM_V); CFHIP_PARAM_X0 is refused as the
 *     reference refuses it (:84-86).  aux: f32 [B][n], what a kind carries between evaluations.
 *       euler_a: d = (x - denoised) / sigma; x += d dt; x += xi sigma_up when flag.  aux is not touched (may be NULL).
 *       heun stage 1: aux = d = (x - denoised) / sigma; x stays; the next input is x_2 = x + d dt.  stage 2: img = x + aux dt (the
 *         same bits), d_2 = (img - denoised) / sigma; x += ((aux + d_2) / 2) dt.  No noise (the reference's draw is unused).
 *       dpmpp_2m: dd = denoised, or [9] denoised - [10] aux when flag; x = [7] x - [8] dd; aux = denoised.  No noise.
 *     xin = bf16(next input * [4]): these samplers feed the UNet img * c_in.  A noise bank is refused for heun and dpmpp_2m.
 *   k_sample_advance: k += 1 and timesteps[0 .. gb) = table[k][0] while k < rows, as f32 (fractional timesteps: default_quantize
 *     off, :219-230) or, with timesteps_int64 != 0, as int64 (:217-218). */
#define CFHIP_KSAMPLE_ROW 12
#define CFHIP_KSAMPLER_EULER_A 0
#define CFHIP_KSAMPLER_HEUN 1
#define CFHIP_KSAMPLER_DPMPP_2M 2
int cfhip_k_sample_step(float* x, float* aux, void* xin, const void* out_c, const void* out_u, float scale, const float* table,
                        int rows, const int* k, const float* noise, int64_t B, int64_t n, int kind, int param, int clip_last,
                        int dup, uint64_t seed, uint64_t offset, void* stream);
int cfhip_k_sample_advance(int* k, const float* table, int rows, void* timesteps, int timesteps_int64, int gb, void* stream);
/* Sampling with a reference: image-to-image and inpainting (ISampler.sample's ref / ref_mask / ref_noise / start_step,
 * samplers/schema.py:153-194).  The `_ref` entry points are the two step entry points above, same operands, same values where
 * the mask is 0, plus:
 *   ref: f32 [B][n], the reference; mask: f32 [B or 1][C or 1][hw] (1 = keep the reference; n = C hw), contiguous and NOT
 *     expanded: element (b, c, pix) is mask[b * mask_bstride + c * mask_cstride + pix], a stride being 0 where the mask has
 *     extent 1 (so (0, 0), (0, hw), (hw, 0) or (n, hw)).
 *   diffusion_sample_step_ref (DDIM / basic; merge_ref, samplers/basic.py:16-35): after row k < steps - 1 has produced the new
 *     state x', the merge the reference performs at the top of step k + 1:
 *         x = mask * (side[k + 1][0] * ref + side[k + 1][1] * nz) + (1 - mask) * x'      (f32, that order, no FMA contraction)
 *     and xin = bf16(x).  The last row does not merge (its image is returned as it is, and clamped with clip_last).
 *     side: f32 [steps][2] = the q-sampler's (w_net, w_noise) of the merge IN FRONT OF each row.  nz by merge_noise_mode:
 *       CFHIP_MERGE_NOISE_PHILOX  (merge_noise NULL) the normals of randn_f32 at counter (seed, offset + (steps + row) * B n / 4
 *                                 + i / 4), row = the row the merge is in front of: disjoint from the starting noise (offset -
 *                                 B n / 4) and from the step draws (offset + row * B n / 4, row < steps) of the same (seed, offset);
 *       CFHIP_MERGE_NOISE_UNIFIED merge_noise f32 [B][n], the same tensor for every merge (use_unified_ref_noise);
 *       CFHIP_MERGE_NOISE_BANK    merge_noise f32 [steps - merge_row0][B][n], entry j for the merge in front of row merge_row0 + j.
 *     merge_row0 (0 <= merge_row0 < steps): the first row the run executes (start_step); no merge in front of an earlier row.
 *   diffusion_sample_merge: the merge in front of row k on its own, x and xin (dup copies) = the merged state: the first
 *     executed step of a run has no preceding step launch to carry it.  A k outside [merge_row0, steps) is a no-op.
 *   k_sample_step_ref (get_denoised_with_reference, samplers/k_samplers.py:185-190): every evaluation's denoised value becomes
 *     mask * ref + (1 - mask) * denoised before the rule uses it (heun: both stages; dpmpp_2m saves the merged value in aux).
 *     No noise, no side table.
 * The step counter stays absolute: a run from start_step s starts k at row s (k_heun: 2 s) and draws what a full run draws there. */
#define CFHIP_MERGE_NOISE_PHILOX 0
#define CFHIP_MERGE_NOISE_UNIFIED 1
#define CFHIP_MERGE_NOISE_BANK 2
int cfhip_diffusion_sample_step_ref(float* x, void* xin, const void* out_c, const void* out_u, float scale, const float* table,
                                    int steps, const int* k, const float* noise, int64_t B, int64_t n, int kind, int param,
                                    float temperature, int clip_last, int dup, uint64_t seed, uint64_t offset, const float* ref,
                                    const float* mask, int64_t mask_bstride, int64_t mask_cstride, int64_t hw, const float* side,
                                    const float* merge_noise, int merge_noise_mode, int merge_row0, void* stream);
int cfhip_diffusion_sample_merge(float* x, void* xin, int steps, const int* k, int64_t B, int64_t n, int dup, uint64_t seed,
                                 uint64_t offset, const float* ref, const float* mask, int64_t mask_bstride, int64_t mask_cstride,
                                 int64_t hw, const float* side, const float* merge_noise, int merge_noise_mode, int merge_row0,
                                 void* stream);
int cfhip_k_sample_step_ref(float* x, float* aux, void* xin, const void* out_c, const void* out_u, float scale, const float* table,
                            int rows, const int* k, const float* noise, int64_t B, int64_t n, int kind, int param, int clip_last,
                            int dup, uint64_t seed, uint64_t offset, const float* ref, const float* mask, int64_t mask_bstride,
                            int64_t mask_cstride, int64_t hw, void* stream);
/* Vector quantisation (csrc/vq.hip): the nearest-code search of VQCodebook.forward (modules/cv/common.py:362-400: sum, einsum,
 * add, argmin over a materialised rows x num_codes f32 distance matrix, then the gather codebook[indices]) as ONE launch that
 * never forms the matrix, for the VQ first stage of latent diffusion (cv/ae/vq.py:63-67, encode; with LDM.preprocess's
 * scale_factor, multimodal/diffusion/ldm.py:183-190, folded into the lookup).
 *   vq_code_sqnorm: out[j] (f32 [N]) = sum_d e_jd^2 of codebook f32 [N][D] (torch.sum(codebook**2, dim=1), common.py:381), one
 *     fmaf chain in d order from 0.  The codebook is frozen under LDM: callers compute this once and keep it.
 *   vq_nearest: z = the [B][D][hw] (channels_last = 0) or [B][hw][D] (channels_last != 0) output of to_embedding, bf16 or f32
 *     (z_is_f32), read in place.  Per pixel score_j = code_sq[j] - 2 dot_j, dot_j the f32 fmaf chain over d = 0 .. D - 1 from 0
 *     (|z|^2 is constant per pixel and left out); indices[b][p] (int64) = the lowest j with the least score (ascending scan,
 *     strict <); z_q[b][d][p] (f32, contiguous [B][D][hw], or NULL) = scale_factor * codebook[idx][d]: one f32 product, the
 *     codebook row bit for bit when scale_factor == 1.  A pixel that holds NaN / inf gets SOME index in [0, N), nothing more.
 *     1 <= D <= CFHIP_VQ_MAX_DIM, N >= 1; anything else is CFHIP_ERR_INVALID.
 *   The codebook streams through LDS cfhip_vq_chunk(D) codes at a time (CFHIP_VQ_LDS_FLOATS floats of [sq_j, e_j..] records; 0
 *   for an unsupported D): a host-side query.  From CFHIP_VQ_TWO_ROWS_MIN_GROUPS workgroups of 128 rows on, a lane holds two
 *   rows instead of one (same arithmetic, same results). */
#define CFHIP_VQ_MAX_DIM 64
#define CFHIP_VQ_LDS_FLOATS 8192
#define CFHIP_VQ_TWO_ROWS_MIN_GROUPS 512
int cfhip_vq_chunk(int D);
int cfhip_vq_code_sqnorm(const float* codebook, float* out, int N, int D, void* stream);
int cfhip_vq_nearest(const void* z, int z_is_f32, int channels_last, const float* codebook, const float* code_sq, int64_t* indices,
                     float* z_q, int64_t B, int D, int64_t hw, int N, float scale_factor, void* stream);
/* Token merging (csrc/tome.hip): tomesd as the reference's SpatialTransformerHooks run it (modules/core/mixed_stacks/api.py:473-589
 * bipartite_soft_matching_random2d, :592-618 compute_merge, :679-685 the block arithmetic), forward only, without the
 * [B][n_src][n_dst] cosine matrix.  x bf16 [B][N][C]; src_idx int32 [n_src] and dst_idx int32 [n_dst] = the token ids of the two
 * sides of the split (api.py:492-528), each ascending, shared by the B samples; n_src + n_dst == N.
 *   tome_match (api.py:536-545): rinv f32 [B][N] (workspace, written first) = 1 / |x_t|, the squares summed in f32, 0 for a zero row
 *     (the reference divides by zero there); node_max f32 [B][n_src], node_idx int32 [B][n_src] = max and lowest arg-max over j of
 *     (dot(x[src_idx[i]], x[dst_idx[j]]) * rinv_src) * rinv_dst: the dot on bf16 MFMA over the raw rows with f32 accumulation, both
 *     inverse norms applied in f32 after it.  Nothing of size n_src * n_dst is written.
 *   tome_select (api.py:546-550, the argsort and its three slices): the r rows of a sample with the largest node_max, ties to the
 *     lowest position, by radix select + prefix sums (no sort, no floating-point atomics, bit-identical between runs).  Merged
 *     rows are ordered [unmerged src, ascending token | dst, ascending token].  Writes row_of_token int32 [B][N] (a merged src
 *     token holds its dst's row), token_of_row int32 [B][N - r], member_off int32 [B][n_dst + 1] and members int32 [B][r]: the
 *     tokens merged into dst j are members[member_off[j] .. member_off[j + 1]), ascending.  cursor int32 [B][n_dst]: workspace.
 *     1 <= r <= n_src.
 *   tome_merge (api.py:552-560): out bf16 [B][N - r][C]: an unmerged row is a copy, a dst row (dst + sum of its members) /
 *     (1 + count), summed in f32 in ascending token order, one rounding (scatter_reduce "mean" with include_self).
 *   tome_unmerge_add (api.py:562-587 and the `+ net` of :682-684): out[b][t] = residual[b][t] + y[b][row_of_token[b][t]], y bf16
 *     [B][N - r][C], residual and out both f32 (out_is_f32 != 0) or both bf16, one f32 add and one rounding; residual NULL: the
 *     plain unmerge.
 * C % 8 == 0, 8 <= C <= CFHIP_TOME_MAX_CHANNELS, N <= CFHIP_TOME_MAX_TOKENS, B <= 65535; anything else is CFHIP_ERR_INVALID. */
#define CFHIP_TOME_MAX_CHANNELS 1280
#define CFHIP_TOME_MAX_TOKENS 65536
int cfhip_tome_match(const void* x, const int* src_idx, const int* dst_idx, float* rinv, float* node_max, int* node_idx, int64_t B,
                     int N, int C, int n_src, int n_dst, void* stream);
int cfhip_tome_select(const float* node_max, const int* node_idx, const int* src_idx, const int* dst_idx, int* row_of_token,
                      int* token_of_row, int* member_off, int* members, int* cursor, int64_t B, int N, int n_src, int n_dst, int r,
                      void* stream);
int cfhip_tome_merge(const void* x, const int* token_of_row, const int* member_off, const int* members, void* out, int64_t B, int N,
                     int C, int n_src, int n_dst, int r, void* stream);
int cfhip_tome_unmerge_add(const void* y, const int* row_of_token, const void* residual, void* out, int out_is_f32, int64_t B, int N,
                           int C, int r, void* stream);
/* dst[b * dst_bs + i] = src[b * src_bs + i] (bf16, i < n, everything a multiple of 4 elements): channel concat /
 * split of NCHW tensors — torch.cat(dim=1) of the UNet skip connections (multimodal/diffusion/unet.py:311-316) */
int cfhip_copy_strided_bf16(const void* src, void* dst, int64_t batch, int64_t n, int64_t src_batch_stride,
                            int64_t dst_batch_stride, void* stream);
/* two of them (same batch count) in one launch: both halves of torch.cat([a, b], dim=1) or of its backward split (unet.py:311-316) */
int cfhip_copy_strided2_bf16(const void* src_a, void* dst_a, int64_t n_a, int64_t src_a_batch_stride, int64_t dst_a_batch_stride,
                             const void* src_b, void* dst_b, int64_t n_b, int64_t src_b_batch_stride, int64_t dst_b_batch_stride,
                             int64_t batch, void* stream);
/* GEGLU (activations.py:150-158): out[m][c] = vg[m][c] * gelu_erf(vg[m][L + c]) for vg bf16 [M][2L]; bwd writes dvg */
int cfhip_geglu_fwd(const void* vg, void* out, int64_t M, int L, void* stream);
int cfhip_geglu_bwd(const void* dy, const void* vg, void* dvg, int64_t M, int L, void* stream);
int cfhip_add_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);
/* bf16 [R,C] -> bf16 [C,R] */
int cfhip_transpose_bf16(const void* src, void* dst, int R, int C, int64_t ld_src, int64_t ld_dst,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * K14  fused Adam / AdamW over a flat fp32 parameter arena (next-row §8f; replaces
 *     torch.optim.Adam(W).step() selected by optimizers.py:29-33)
 *   p, g, m, v: f32 [n].  p_bf16 (may be NULL): refreshed bf16 copy of the parameters for the
 *   next forward.  grad_scale multiplies g first (1/world_size for DDP-mean, clip coefficient).
 *   step >= 1 (bias correction).  decoupled != 0 -> AdamW.  The betas arrive as double: the kernel multiplies with
 *   their float values, the bias corrections 1 - beta1^t and 1 / sqrt(1 - beta2^t) are taken in double from the
 *   betas as given — what torch.optim and FusedAdam's record do (from the float betas 1 / sqrt(1 - beta2^t) was
 *   6.5e-6 away from the record's at t = 1, beta2 = 0.999).
 * ------------------------------------------------------------------------------------------ */
int cfhip_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                    double beta1, double beta2, float eps, float weight_decay, int decoupled, int step,
                    float grad_scale, void* stream);
/* same update, step-dependent scalars read from device memory so the launch can be replayed from a
 * captured hipGraph: hyper[0..7] = lr, beta1, beta2, eps, weight_decay, 1-beta1^t, 1/sqrt(1-beta2^t),
 * grad_scale (f32, device). */
int cfhip_adam_step_dev(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                        const float* hyper, int decoupled, void* stream);
/* EMA of the parameters (modules/common.py:126-137): ema = (1 - decay) * p + decay * ema over a flat f32 buffer
 * (16-byte aligned); two rounded products + one rounded sum like the reference's expression: bit-exact.
 * the reference clones every parameter every step. */
int cfhip_ema_update(float* ema, const float* p, int64_t n, float one_minus_decay, float decay, void* stream);
/* Implicit-GEMM 3x3 / stride 1 / padding 1 convolution on NHWC bf16 activations (F.conv2d reached from Conv2d.forward,
 * reference convs/basic.py:160-177, as used 61 times by the DDPM UNet, unet.py:76-322): Y[p][co] = bias[co] +
 * sum_{ky,kx,c} X[p + (ky-1)*W + (kx-1)][c] * Wk[co][(ky*3+kx)*Cin + c] over the pixels p of B images of H x W, taps
 * outside the image contribute zero.  X [B*H*W][Cin], Wk [Cout][9*Cin] (tap-major, channel-minor), Y [B*H*W][Cout],
 * all bf16; bias f32 [Cout] or NULL.  Cin % 32 == 0, Cout % 8 == 0.  No im2row matrix is materialised: each K-step of
 * the MFMA GEMM gathers 32 channels of one tap straight from X.  The input gradient is the same call with dY in place
 * of X and the filters rotated by 180 degrees and transposed: Wk'[c][(ky*3+kx)*Cout + co] = W[co][c][2-ky][2-kx].
 * Shapes with few output tiles split the reduction (deterministic ordered reduce of fp32 partials): pass
 * cfhip_conv3x3_workspace() bytes of scratch (0 when the shape does not split). */
size_t cfhip_conv3x3_workspace(int B, int H, int W, int Cin, int Cout);
int cfhip_conv3x3_nhwc_bf16(const void* X, const void* Wk, const float* bias, void* Y, int B, int H, int W, int Cin,
                            int Cout, void* workspace, size_t workspace_bytes, void* stream);
/* Weight gradient of the same convolution without an im2row matrix: dW[co][c][ky][kx] (+)= sum_p dY[p][co] *
 * X[p + (ky-1)*W + (kx-1)][c] (taps outside the image contribute zero), f32 in the reference's [Cout][Cin][3][3] layout
 * (`accumulate` != 0: added to dW).  dY [B*H*W][Cout], X [B*H*W][Cin] bf16 NHWC; Cin % 8 == 0, Cout % 8 == 0, H, W >= 2,
 * B*H*W*max(H, W) < 2^32.  bias_grad (f32 [Cout] or NULL) (+)= colsum(dY).  The GEMM writes fp32 partial sums per K slice
 * ([split_k][Cout][9*Cin], tap-major) into the workspace (cfhip_conv3x3_wgrad_workspace() bytes, needed for every
 * split_k >= 1); a second pass adds them in a fixed order and writes the filter layout: deterministic. */
size_t cfhip_conv3x3_wgrad_workspace(int Cin, int Cout, int split_k);
int cfhip_conv3x3_wgrad_nhwc_bf16(const void* dY, const void* X, float* dW, int accumulate, float* bias_grad,
                                  int bias_grad_accumulate, int B, int H, int W, int Cin, int Cout, int split_k,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* Filter repacking for the two calls above, w bf16 [Cout][Cin][3][3] (Cin % 8 == 0):
 *   rotate == 0: out[co][(ky*3+kx)*Cin + c]        = w[co][c][ky][kx]       ([Cout][9*Cin], the forward's Wk)
 *   rotate != 0: out[c][(ky*3+kx)*Cout + co]       = w[co][c][2-ky][2-kx]   ([Cin][9*Cout], the input gradient's Wk') */
int cfhip_conv3x3_pack_filters(const void* w, void* out, int Cout, int Cin, int rotate, void* stream);
/* The same for 1 .. CFHIP_PACK_GROUP_MAX filter banks in one launch: `table` is a HOST array of 5 int64 per problem {w, out, Cout, Cin, rotate} (the pointers
 * travel in the kernel arguments).  What a model calls once at the top of its forward instead of two packs per convolution
 * (functional.prepack_convs; reference: every `conv_nd(2, ..., 3, padding=1)` of unet.py / residual.py reaches F.conv2d with its own weight). */
#define CFHIP_PACK_GROUP_MAX 64 /* problems per call */
int cfhip_conv3x3_pack_filters_grouped(const int64_t* table, int count, void* stream);
/* Direct 3x3 convolution for few channels, without the im2row matrix, LDS or barriers (csrc/conv_direct.hip): the ControlNet hint block
 * (reference multimodal/diffusion/unet.py:441-457: `conv_nd(2, hint, 16, 3, padding=1)` ... `conv_nd(2, 32, 96, 3, padding=1, stride=2)`
 * on the pixel-space hint, each reaching F.conv2d), pad 1, stride 1 or 2.
 *   conv3x3_direct_pack: f32 filter w [Cout][Cin][3][3] -> bf16 wp[N][Kp], k = tap * Cp + c, tap = ky * 3 + kx; Cp = the channels of the
 *     kernel's INPUT rounded up to a multiple of 8, Kp = 9 Cp rounded up to a multiple of 32, every padded position zero.
 *       mode 0 (forward):        N = Cout,                    Cp from Cin,  wp[co][tap Cp + c] = w[co][c][ky][kx]
 *       mode 1 (input gradient): N = Cin rounded up to 8,     Cp from Cout, wp[c][tap Cp + co] = w[co][c][2 - ky][2 - kx]
 *   conv3x3_direct_bf16: x, y NHWC bf16, bias f32 [N] or null; Cp in {8, 16, 24, 32, 48, 64, 80, 96} (the hint block uses
 *     8, 16, 32 and 96; the others are what `functional.direct_conv_ok` also admits), N a multiple of 8 up to 96; (H, W) is the image of
 *     the FORWARD's input in both modes, Ho = (H - 1) / stride + 1.
 *       mode 0: x [B][H][W][Cp] -> y [B][Ho][Wo][N] = bias + sum over taps inside the image
 *       mode 1: x = dY [B][Ho][Wo][Cp] -> y = dX [B][H][W][N]: filter tap (ky, kx) of pixel (iy, ix) reads dY[(iy + 1 - ky) / s][(ix + 1 - kx) / s]
 *               where both numerators are non-negative and divisible by s and the quotients are inside dY
 * and the SiLU between those convolutions, element-wise on bf16 (`nn.SiLU()` of the same Sequential; silu_f32 is the f32 form); n = 0
 * launches nothing and returns 0, here and in cfhip_scale_bf16. */
int cfhip_conv3x3_direct_pack(const float* w, void* wp, int Cout, int Cin, int mode, void* stream);
int cfhip_conv3x3_direct_bf16(const void* x, const void* wp, const float* bias, void* y, int B, int H, int W, int Cp, int N,
                              int stride, int mode, void* stream);
int cfhip_silu_bf16_fwd(const void* x, void* y, int64_t n, void* stream);
int cfhip_silu_bf16_bwd(const void* dy, const void* x, void* dx, int64_t n, void* stream);
/* y = bf16(scale * x), bf16 [n]: a ControlNet output times its control scale (reference ddpm.py:413-419, `c * scale`); its gradient is
 * the same call on dy. */
int cfhip_scale_bf16(const void* x, void* y, int64_t n, float scale, void* stream);
/* Dense-block 3x3 / stride 1 / padding 1 convolution on bf16 NHWC rows with ROW STRIDES on both sides (csrc/conv_dense.hip): the RRDB
 * upscaler (reference cflearn/modules/cv/translator/rrdb.py:15-29, the five `nn.Conv2d(..., 3, 1, 1)` of a ResidualDenseBlock over
 * `torch.cat((inp, net1, ...), 1)` with `self.lrelu` and `net * 0.2 + inp`; rrdb.py:39-44 the RRDB's own `net * 0.2 + inp`; rrdb.py:77-85
 * and :95-101 conv_first, conv_body with `net + body`, conv_up1 / conv_up2 behind `F.interpolate(scale_factor=2, mode="nearest")`,
 * conv_hr and conv_last).  A dense block keeps [inp, net1 .. net4] in ONE buffer [B H W][192] and never concatenates:
 *   x: channel 0 of a bf16 buffer [B H W][ld_in]; the channel prefix [0, Cin) of every row is read.  Cin % 8 == 0, 8 <= Cin <= 192.
 *   wp: bf16 [N][Kp], the layout of cfhip_conv3x3_direct_pack mode 0 (k = tap Cin + c, Kp = 9 Cin rounded up to 32); a filter bank with
 *     fewer than N rows is packed into the first rows of a zeroed [N][Kp] (conv_last: 3 of 16).  N in {16, 32, 64}.
 *   y: the first output channel of a bf16 buffer [B Ho Wo][ld_out]; n_store <= N channels per row are written and nothing else.
 *     out_f32_nchw != 0: y is f32 [B][n_store][Ho][Wo] instead (the layout RRDBNet.forward returns; ld_out is ignored).
 *   bias: f32 [n_store] or NULL.  f32 accumulation over k in a fixed order: no split reduction, no atomics, bit-identical run to run.
 *   epilogue, in f32, every operation rounded on its own as the reference's eager ops are, one rounding to the output type:
 *     CFHIP_DENSE_EPI_NONE   v = acc + bias
 *     CFHIP_DENSE_EPI_LRELU  v > 0 ? v : slope v                      (rrdb.py:24-27, :99-101)
 *     CFHIP_DENSE_EPI_RES1   s1 v + r1                                (rrdb.py:29 with s1 = 0.2; rrdb.py:97 with s1 = 1)
 *     CFHIP_DENSE_EPI_RES2   (s1 v + r1) s2 + r2                      (rrdb.py:29 then rrdb.py:44: conv5 of an RRDB's third block)
 *     r1 / r2: bf16 rows [B Ho Wo] with row strides ld_r1 / ld_r2 (multiples of 8), n_store channels each.
 *   up2 != 0: the input is the nearest-neighbour 2x upsampling of x [B][H][W] (rrdb.py:88), never materialised: Ho = 2 H, Wo = 2 W and
 *     output pixel (oy, ox) reads x[(oy - 1 + ky) >> 1][(ox - 1 + kx) >> 1] for taps inside [0, 2H) x [0, 2W), zero outside; else
 *     Ho = H, Wo = W.
 * Pixel offsets are 64-bit.  Every pointer is 16-byte aligned, ld_in and ld_out are multiples of 8.  A call whose output bytes meet the
 * bytes it reads (x's prefix, r1, r2) is refused before any launch — the taps of neighbouring pixels would race — except the dense
 * block's own case: the same row grid (equal strides, up2 == 0) with the written columns clear of the read ones.
 * One workgroup per CFHIP_DENSE_TILE_H x CFHIP_DENSE_TILE_W output pixels. */
#define CFHIP_DENSE_TILE_H 8
#define CFHIP_DENSE_TILE_W 32
#define CFHIP_DENSE_EPI_NONE 0
#define CFHIP_DENSE_EPI_LRELU 1
#define CFHIP_DENSE_EPI_RES1 2
#define CFHIP_DENSE_EPI_RES2 3
int cfhip_conv3x3_dense_bf16(const void* x, const void* wp, const float* bias, void* y, const void* r1, const void* r2, int B, int H, int W,
                             int Cin, int N, int n_store, int64_t ld_in, int64_t ld_out, int64_t ld_r1, int64_t ld_r2, int epilogue,
                             float slope, float s1, float s2, int up2, int out_f32_nchw, void* stream);
/* The input of the RRDB upscaler (rrdb.py:47-55 `pixel_unshuffle` and the layout change in front of conv_first, rrdb.py:91-95):
 * x [B][C][H][W] f32 (x_is_f32 != 0) or bf16 -> y bf16 NHWC [B][H / s][W / s][Cp], y[b][oy][ox][c s^2 + dy s + dx] =
 * x[b][c][oy s + dy][ox s + dx]; Cp = C s^2 rounded up to a multiple of 8, the padding channels zero.  s in {1, 2, 4}, H % s == W % s == 0. */
int cfhip_pixel_unshuffle_nhwc(const void* x, int x_is_f32, void* y, int64_t B, int C, int H, int W, int s, void* stream);
/* One idle wavefront for `microseconds` (1..100000) on `stream`.  Host-side stream self-check only (two streams
 * that share a ROCclr hardware queue run it back to back; the side streams of the backward pass and the RCCL
 * stream must not share the compute stream's queue -- reference counterpart: none, torch DDP owns its streams). */
int cfhip_spin(int microseconds, void* stream);
/* sum of squares of g (f32 [n]) into out[0] (+= ; caller zeroes) — gradient-norm clipping */
int cfhip_sumsq_f32(const float* g, float* out, int64_t n, void* stream);

/* softmax cross-entropy on f32 logits [B,C] with int64 labels [B]: loss_sum (f32[1], caller
 * zeroes) += sum_b CE_b ; dlogits (f32 [B,C]) = (softmax - onehot) * grad_scale.
 * (losses/basic.py:126-141; integer label gather is exact.) */
int cfhip_softmax_xent(const float* logits, const int64_t* labels, float* loss_sum, float* dlogits,
                       int B, int C, float grad_scale, void* stream);
/* focal loss (losses/basic.py:170-206, the examples' default): p = softmax(z) + eps,
 * L_b = -log(p_y) (1 - p_y)^gamma; loss_sum += sum_b L_b; dlogits = grad_scale * dL/dz. */
int cfhip_softmax_focal(const float* logits, const int64_t* labels, float* loss_sum, float* dlogits,
                        int B, int C, float gamma, float eps, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8 general form: Conv2d (groups 1) = im2row + K1 GEMM (convs/basic.py:104-177 -> F.conv2d)
 *   conv_im2row: x f32/bf16 [B,C,H,W] -> rows bf16 [B*Ho*Wo][Kp], k = (c, ky, kx), zero padding,
 *     columns K..Kp-1 zero (Kp = K rounded up to a multiple of 8: the GEMM operand rule), so
 *     y_rows = rows x W[Cout][Kp]^T (+bias) is one cfhip_gemm_bf16 call and dW the (tn) GEMM of
 *     the same rows;  Ho = (H + 2 pad - dil (kh - 1) - 1) / stride + 1.
 *   conv_row2im: dx bf16 [B,C,H,W] = gather-sum of drows bf16 [B*Ho*Wo][Kp] (= dY_rows x W): every
 *     input pixel sums its <= kh*kw contributions — no atomics, deterministic.
 *   transpose_batched: src f32/bf16 [batch][R][C] -> dst bf16 [batch][C][R]: NCHW <-> token-major.
 * K9/K10: BatchNorm over (B, inner) per channel of x [B][C][inner] (norms.py:20-27,90-93 ->
 *   nn.BatchNorm1d/2d): training = batch statistics (biased variance), running statistics updated
 *   with `momentum` and the UNBIASED variance; eval = running statistics.  y bf16, mean/rstd f32 [C]
 *   saved for backward; bwd: dgamma/dbeta f32 [C] ((+)= with accumulate), dx bf16 (NULL to skip).
 * LeakyReLU (slope 0 = ReLU; activations.py "leaky_relu_0.2", "ReLU"), AdaptiveAvgPool2d((1,1))
 *   (cv/encoder/vanilla.py:144): x [BC][inner] -> y [BC].
 * ------------------------------------------------------------------------------------------ */
int cfhip_conv_im2row(const void* x, int x_is_f32, void* rows, int B, int C, int H, int W, int kh,
                      int kw, int stride, int pad, int dil, int Kp, void* stream);
int cfhip_conv_row2im(const void* drows, void* dx, int B, int C, int H, int W, int kh, int kw,
                      int stride, int pad, int dil, int Kp, void* stream);
/* The same gather and its transpose with a zero padding of its own on each side: pad_t / pad_l rows / columns before the
 * image, pad_b / pad_r after it, Ho = (H + pad_t + pad_b - dil (kh - 1) - 1) / stride + 1.  The encoder's down-sampling
 * (cv/encoder/attn.py:14-28: F.pad(net, (0, 1, 0, 1)) then a 3x3 stride-2 convolution with padding 0) is pad_t = pad_l = 0,
 * pad_b = pad_r = 1: one gather plus the GEMM, no padded copy of the image. */
int cfhip_conv_im2row_pad(const void* x, int x_is_f32, void* rows, int B, int C, int H, int W, int kh, int kw, int stride,
                          int pad_t, int pad_b, int pad_l, int pad_r, int dil, int Kp, void* stream);
int cfhip_conv_row2im_pad(const void* drows, void* dx, int B, int C, int H, int W, int kh, int kw, int stride, int pad_t,
                          int pad_b, int pad_l, int pad_r, int dil, int Kp, void* stream);
int cfhip_transpose_batched(const void* src, int src_is_f32, void* dst, int batch, int R, int C,
                            void* stream);
int cfhip_batchnorm_fwd(const void* x, int x_is_f32, const float* gamma, const float* beta, void* y,
                        float* mean, float* rstd, float* running_mean, float* running_var, int B, int C,
                        int inner, float eps, float momentum, int training, void* stream);
int cfhip_batchnorm_bwd(const void* dy, const void* x, int x_is_f32, const float* gamma,
                        const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta,
                        int B, int C, int inner, int accumulate, int training, void* stream);
int cfhip_leaky_relu_fwd(const void* x, void* y, int64_t n, float slope, void* stream);
int cfhip_leaky_relu_bwd(const void* dy, const void* x, void* dx, int64_t n, float slope, void* stream);
int cfhip_avgpool_fwd(const void* x, void* y, int64_t BC, int inner, void* stream);
int cfhip_avgpool_bwd(const void* dy, void* dx, int64_t BC, int inner, void* stream);

/* ------------------------------------------------------------------------------------------
 * UNet residual-block pieces (convs/residual.py:86-253, multimodal/diffusion/unet.py:52-74)
 *   groupnorm: y = [SiLU](GroupNorm_G(x + add[b][c])) over x f32/bf16 [B][C][inner], statistics per
 *     (b, group) in fp32 (mean / rstd f32 [B*G] saved); `add` (f32 [B][C], may be NULL) is the
 *     time-embedding term `Linear(SiLU(t))[:, :, None, None]` the reference adds in front of norm2.
 *     bwd: dx bf16, per-batch partial dgamma / dbeta f32 [B][C] (sum them over B with
 *     cfhip_colsum / a column reduce), dadd f32 [B][C] = sum_inner dx (NULL when there was no add).
 *   silu_f32: the activation on the [B, 1280] time embedding;  upsample2 / avgpool2: nearest x2
 *     (F.interpolate(scale_factor=2, "nearest")) and 2x2 average pooling of bf16 [BC][H][W]
 *     (H, W = the SMALL size in both);  timestep_embedding: [cos(t f_i) | sin(t f_i)], f32.
 * ------------------------------------------------------------------------------------------ */
/* gamma / beta: f32 [C], or ONE AFFINE PER SAMPLE, f32 [B][C], when affine_batch_stride == C (0: the plain form).
 * `norm2(net) * (1 + scale) + shift` of the scale-shift residual block (convs/residual.py:236-239) is GroupNorm with
 * gamma_eff[b][c] = gamma[c] (1 + scale[b][c]), beta_eff[b][c] = beta[c] (1 + scale[b][c]) + shift[b][c]; bwd then leaves
 * d gamma_eff / d beta_eff in dgamma_part / dbeta_part [B][C] (no reduction over B).
 * splits <= 1: one workgroup per (sample, group), workspace may be NULL — 8 elements per lane when inner % 8 == 0, the tensors
 * are 16-byte aligned and (bwd) C / G <= CFHIP_GN_MAX_CG, one element per lane otherwise.  splits 2 .. 64 (<= inner / 8): every
 * (sample, group) cut into that many slices along `inner`, one workgroup each — for few samples (B * G workgroups do not fill
 * 256 CUs: the batch-1 256^2 UNet step); it REQUIRES those three conditions.  Statistics: per-slice (mean, M2) merged in slice
 * order (Chan's update), so results do not depend on scheduling.  workspace: f32, B * G * splits * 2 (fwd) /
 * B * G * splits * 3 * (C / G) (bwd) elements, owned by the caller. */
#define CFHIP_GN_MAX_CG 128 /* channels per group of the backward's 8-per-lane and split forms */
int cfhip_groupnorm_fwd(const void* x, int x_is_f32, const float* add, const float* gamma, const float* beta,
                        void* y, float* mean, float* rstd, int B, int C, int G, int inner, float eps, int silu,
                        int affine_batch_stride, int splits, float* workspace, void* stream);
int cfhip_groupnorm_bwd(const void* dy, const void* x, int x_is_f32, const float* add, const float* gamma,
                        const float* beta, const float* mean, const float* rstd, void* dx, float* dgamma_part,
                        float* dbeta_part, float* dadd, int B, int C, int G, int inner, int silu,
                        int affine_batch_stride, int splits, float* workspace, void* stream);
int cfhip_silu_f32_fwd(const float* x, float* y, int64_t n, void* stream);
int cfhip_silu_f32_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);
/* The per-block time-embedding projections of the UNet's residual blocks, every block in ONE launch (replaces `self.time_embedding`
 * = Sequential(SiLU, Linear) of each ResidualBlockWithTimeEmbedding: reference convs/residual.py:185-191,226-239, unet.py:154-190).
 *   out_i[b, :] = Linear_i(SiLU(emb[b, :])), i < count <= CFHIP_TIME_PROJ_MAX, emb f32 [B, K] (K % 32 == 0, K <= 2048) shared by all problems; bf16 SiLU(emb)
 *   and bf16 weights, f32 accumulation and output (what the per-block GEMMs computed).  `table`: a HOST array of 4 int64 per problem —
 *   forward {weight bf16 [N, K] (16-byte aligned), bias f32 [N] or 0, out f32 [B, N], N}; backward {weight, dY f32 [B, N] or 0 (no gradient
 *   for that output), bf16 copy of dY [B, N] to write or 0, N}.  t_bf16: SiLU(emb) as bf16 [B, K] (out; the weight-gradient GEMMs' operand).
 *   backward: d_emb[b, k] = SiLU'(emb) * sum_i sum_n bf16(dY_i[b, n]) W_i[n, k]: per-64-column partial sums in `partial` (f32,
 *   (sum_i ceil(N_i / 64)) * ceil8(B) * K elements, caller-owned), summed in block order: deterministic, no atomics. */
#define CFHIP_TIME_PROJ_MAX 32 /* problems per call */
int cfhip_time_proj_fwd(const float* emb, int B, int K, const int64_t* table, int count, void* t_bf16, void* stream);
int cfhip_time_proj_bwd(const float* emb, int B, int K, const int64_t* table, int count, float* partial, float* d_emb, void* stream);
int cfhip_upsample2_fwd(const void* x, void* y, int64_t BC, int H, int W, void* stream);
int cfhip_upsample2_bwd(const void* dy, void* dx, int64_t BC, int H, int W, void* stream);
int cfhip_avgpool2_fwd(const void* x, void* y, int64_t BC, int Ho, int Wo, void* stream);
int cfhip_avgpool2_bwd(const void* dy, void* dx, int64_t BC, int Ho, int Wo, void* stream);
/* NHWC forms (round 5): the UNet keeps its activations as the rows the implicit-GEMM convolutions read and write — bf16 [B][H * W][C],
 * C % 8 == 0 — instead of hopping NCHW <-> NHWC around every convolution.
 *   groupnorm_nhwc: nn.GroupNorm (+ the per-(b, c) additive term in front, + SiLU behind) of convs/residual.py:194,226-247 on such rows;
 *     `splits` slices of rows per sample (one workgroup each), workspace = cfhip_groupnorm_nhwc_workspace(...) bytes;
 *     mean / rstd f32 [B * G]; bwd: dgamma_part / dbeta_part f32 [B][C] (per-sample sums: the caller reduces over B), dadd f32 [B][C]
 *     (with `add`); gamma / beta [C], or [B][C] with affine_batch_stride == C (the scale-shift norm); deterministic, no atomics.
 *   upsample2_nhwc: F.interpolate(scale_factor=2, mode="nearest") (residual.py:147) and its gradient; H, W = the small size. */
size_t cfhip_groupnorm_nhwc_workspace(int B, int C, int G, int splits, int backward, int with_add);
int cfhip_groupnorm_nhwc_fwd(const void* x, const float* add, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                             int B, int C, int G, int inner, float eps, int silu, int affine_batch_stride, int splits, float* workspace,
                             void* stream);
int cfhip_groupnorm_nhwc_bwd(const void* dy, const void* x, const float* add, const float* gamma, const float* beta, const float* mean,
                             const float* rstd, void* dx, float* dgamma_part, float* dbeta_part, float* dadd, int B, int C, int G, int inner,
                             int silu, int affine_batch_stride, int splits, float* workspace, void* stream);
int cfhip_upsample2_nhwc_fwd(const void* x, void* y, int64_t B, int H, int W, int C, void* stream);
int cfhip_upsample2_nhwc_bwd(const void* dy, void* dx, int64_t B, int H, int W, int C, void* stream);
/* nn.ReflectionPad2d in front of F.conv2d (reference convs/basic.py:61-75,114-115: Conv2d(padding="reflection[N]")):
 *   fwd: x [BC][H][W] (bf16, or f32 when x_is_f32) -> y bf16 [BC][H + pt + pb][W + pl + pr], mirrored without repeating the border;
 *   bwd: dx bf16 [BC][H][W] = gather of the <= 9 positions of dy that mirror onto each input pixel (deterministic).
 * Every pad is >= 0 and smaller than the extent it mirrors (torch's rule). */
int cfhip_reflect_pad2d_fwd(const void* x, int x_is_f32, void* y, int64_t BC, int H, int W, int pl, int pr, int pt, int pb,
                            void* stream);
int cfhip_reflect_pad2d_bwd(const void* dy, void* dx, int64_t BC, int H, int W, int pl, int pr, int pt, int pb, void* stream);
/* out[d] (+)= sum_r x[r][d] for a dense f32 [R][D] matrix (per-batch partials -> parameter gradient) */
int cfhip_colreduce_f32(const float* x, float* out, int R, int D, int accumulate, void* stream);
/* two [R, D] matrices into two outputs in one launch (GroupNorm's dgamma / dbeta partial sums: norms.py nn.GroupNorm's weight / bias gradients) */
int cfhip_colreduce2_f32(const float* x_a, float* out_a, const float* x_b, float* out_b, int R, int D, int accumulate, void* stream);
int cfhip_timestep_embedding(const int64_t* t, float* out, int B, int dim, float max_period, void* stream);
/* the same for float timesteps, arg = t[b] * freq (multimodal/diffusion/unet.py:52-74: `timesteps[:, None].float() * frequency`;
 * the sigma-space samplers' interpolated timesteps, samplers/k_samplers.py:219-230) */
int cfhip_timestep_embedding_f32(const float* t, float* out, int B, int dim, float max_period, void* stream);


/* ------------------------------------------------------------------------------------------
 * CLIP text tower index work (multimodal/clip.py:209-256) — gathers are bit-exact
 *   embedding_fwd: out[n][:] = table[indices[n]][:] (+ pos[n % T][:]) — nn.Embedding lookup fused with
 *     the learned positional add (mixed_stacks/api.py:209-228); also the EOT pooling
 *     `net[arange(B), indices.argmax(-1)]` with table = the [B*T, D] stream and indices = b*T + argmax.
 *     table / pos f32, indices int64, out f32 or bf16, D % 4 == 0.
 *   embedding_bwd: dtable[indices[n]][:] += dy[n][:] (f32 atomics; caller zeroes / owns dtable;
 *     rows equal to padding_idx are skipped like nn.Embedding(padding_idx=...)).
 *   l2norm: y = x / ||x||_2 per f32 row (cftool.array.l2_normalize, no epsilon); inv_norm saved.
 * ------------------------------------------------------------------------------------------ */
int cfhip_embedding_fwd(const float* table, const int64_t* indices, const float* pos, void* out,
                        int out_is_f32, int64_t N, int D, int T, int64_t V, void* stream);
int cfhip_embedding_bwd(const void* dy, int dy_is_f32, const int64_t* indices, float* dtable, int64_t N,
                        int D, int64_t V, int64_t padding_idx, void* stream);
int cfhip_l2norm_fwd(const float* x, float* y, float* inv_norm, int64_t N, int D, void* stream);
int cfhip_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int64_t N, int D,
                     void* stream);
/* Similarity logits of the CLIP towers in fp32 (IPerceptor.forward, multimodal/schema.py:25-30:
 * `logit_scale.exp() * image_features @ text_features.t()`) and the products of its backward:
 * C[m][n] = alpha * alpha_dev[0] * sum_k A(m,k) * B(n,k), A(m,k) = a_trans ? A[k*lda + m] : A[m*lda + k] (B likewise),
 * C dense [M][N]; alpha_dev (device scalar, e.g. exp(logit_scale)) may be NULL.  fp32 FMA in k order: the operands are
 * not rounded to bf16.  dot: out[0] += sum a[i]*b[i] (d logit_scale = sum(dlogits * logits); caller zeroes).
 * The contrastive loss built on them (contrastive.py) has no counterpart in the reference: parity unpinned. */
int cfhip_sgemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int64_t lda, int64_t ldb,
                    int a_trans, int b_trans, const float* alpha_dev, float alpha, void* stream);
int cfhip_dot_f32(const float* a, const float* b, float* out, int64_t n, void* stream);


/* ------------------------------------------------------------------------------------------
 * A12  dropout / stochastic depth (nn.Dropout at channel_mixers.py:30-41, mixed_stacks/api.py:130-158,
 *      ml_encoder.py:60-70, mappings.py:60-80; DropPath at modules/core/customs.py:429-446)
 *   dropout: y[i] = keep_i ? x[i] * s : 0 with s = 1 / (1 - p) in x's dtype (bf16 tensors: s rounded to bf16 first,
 *     as torch forms its noise `mask / (1 - p)` in the input's dtype) — bit-equal to torch given the mask.  `p` is a
 *     double because torch forms 1 - p in double and rounds THAT to f32: s = 1.0f / (float)(1.0 - p).  keep_i = mask_in[i] != 0 when mask_in is given (one byte per element: parity tests inject the
 *     reference's mask), else u_i >= (float)p with u from Philox4x32-10 keyed by `seed`, counter = offset + i / 4, lane i % 4
 *     — a pure function of (seed, offset, i), so the BACKWARD is the same call on dy with the same (seed, offset):
 *     no mask tensor is stored.  A call consumes ceil(n / 4) counters.  mask_out (optional) receives the mask.
 *     x / y bf16 or f32, 16-byte aligned; 0 <= p < 1.
 *   drop_path_mask: mask[b] = floor(keep_prob + u_b), 0 or 1 (customs.py:439-441), u_b from the same generator
 *     (counter = offset + b / 4).  drop_path: y[b][:] = (x[b][:] / keep_prob) * mask[b] — the reference's two
 *     roundings (customs.py:442) with a true IEEE division, `inner` elements per sample (inner % 4 == 0), bf16 or
 *     f32; bit-equal to the reference given the mask.  Its backward is the same call on dy.
 * ------------------------------------------------------------------------------------------ */
int cfhip_dropout(const void* x, void* y, int is_f32, int64_t n, double p, uint64_t seed, uint64_t offset,
                  const uint8_t* mask_in, uint8_t* mask_out, void* stream);
int cfhip_drop_path_mask(float* mask, int64_t B, float keep_prob, uint64_t seed, uint64_t offset, void* stream);
int cfhip_drop_path(const void* x, void* y, int is_f32, const float* mask, float keep_prob, int64_t B, int64_t inner,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA adapters of Linear layers (csrc/lora.hip).  Replace the adapter arithmetic of LoRALinearHook.after_forward,
 *   modules/core/hijacks.py:157-166 — `lora_down(inp)` (nn.Linear, :159), `lora_up(net)` (:161), `dropout(net)` (:162),
 *   `scale * net` (:164), `out + net` (:165) — and the autograd backward of those ATen ops.  A [r][K] = lora_down.weight,
 *   Bm [N][r] = lora_up.weight, 1 <= r <= 64 (padded to the MFMA width inside the kernels, never in memory); bf16 operands,
 *   f32 accumulation, no atomics: results are reproducible bit for bit.  `mask` is cfhip_dropout's keep mask over the
 *   contiguous [rows][cols] index space of the wide tensor (element i: counter offset + i / 4, word i % 4, keep = u >= p;
 *   a call covers ceil(rows * cols / 4) counters) and is regenerated from (seed, offset) by every kernel that needs it; with
 *   p > 0 `scale` is multiplied by 1 / (1 - p) in f32; p == 0 skips the generator.  Wide dimensions are multiples of 8,
 *   wide tensors 16-byte aligned.
 *   lora_down:   h[m][c] (bf16 [M][r], contiguous) = scale * sum_k (mask . x)[m][k] * F(c, k);  x bf16 [M][K] (ldx), read once.
 *                f_trans == 0: F(c, k) = f[c * ldf + k]  (forward: f = A, p = 0 -> h = x A^T, hijacks.py:159)
 *                f_trans != 0: F(c, k) = f[k * ldf + c]  (backward: x = dy [M][N], f = Bm -> dh = s (mask . dy) Bm)
 *   lora_up_add: y[m][n] += scale * mask[m][n] * sum_c h[m][c] * F(n, c);  y bf16 or f32 [M][N] (ldy), one read-modify-write
 *                pass, dropped positions keep their bits.
 *                f_trans == 0: F(n, c) = f[n * ldf + c]  (forward: f = Bm, on the base GEMM's output before any activation, :161-165)
 *                f_trans != 0: F(n, c) = f[c * ldf + n]  (backward: h = dh, f = A, y = the dX the base GEMM wrote, p = 0)
 *   lora_wgrad:  out (+)= scale * sum_m (mask . t)[m][j] * u[m][c];  t bf16 [M][J] (ldt), u bf16 [M][r] contiguous, out f32
 *                [J][r] (out_trans == 0: dBm with t = dy, u = h) or [r][J] (out_trans != 0: dA with t = x, u = dh, p = 0).
 *                The reduction over M is cut into row splits whose f32 partial sums go to `workspace`
 *                (>= cfhip_lora_wgrad_workspace(M, J, r) bytes) and are added in split order by a second kernel.
 * ------------------------------------------------------------------------------------------ */
int cfhip_lora_down(const void* x, const void* f, void* h, int M, int K, int r, int64_t ldx, int64_t ldf, int f_trans,
                    float scale, float p, uint64_t seed, uint64_t offset, void* stream);
int cfhip_lora_up_add(const void* h, const void* f, void* y, int y_is_f32, int M, int N, int r, int64_t ldf, int64_t ldy,
                      int f_trans, float scale, float p, uint64_t seed, uint64_t offset, void* stream);
size_t cfhip_lora_wgrad_workspace(int M, int J, int r);
int cfhip_lora_wgrad(const void* t, const void* u, float* out, int M, int J, int r, int64_t ldt, int out_trans,
                     int accumulate, float scale, float p, uint64_t seed, uint64_t offset, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA adapters of Conv2d layers (csrc/lora.hip).  Replace the adapter arithmetic of LoRAConvHook,
 *   modules/core/hijacks.py:208-266 — `lora_down` a k x k nn.Conv2d Cin -> r with the base layer's stride and padding (:231-240),
 *   `lora_up` a 1x1 nn.Conv2d r -> Cout (:241-249), applied by ILoRAMappingHook.after_forward (:157-166) — and the autograd
 *   backward of those convolutions.  Activations are NHWC rows [B * H * W][C] (bf16); in that layout every 1x1 piece is one of
 *   cfhip_lora_down / cfhip_lora_up_add / cfhip_lora_wgrad above (the dropout mask lives there, on the up term only).  The three
 *   entry points below are the 3x3 / pad 1 / stride 1 or 2 down factor: Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1,
 *   nbr(b, oy, ox, ky, kx) = (b, oy * stride + ky - 1, ox * stride + kx - 1), zero outside the image.  `f` is the bf16 copy of
 *   lora_down.weight in the parameter's own layout f[c][ci][ky][kx] = f[((c * C + ci) * 3 + ky) * 3 + kx], contiguous; it is
 *   permuted to (ky, kx, ci) order inside the kernels, no packed copy exists.  C % 8 == 0, 1 <= r <= 64 (padded to the MFMA
 *   width inside the kernels only), B * H * W < 2^31; bf16 operands, f32 accumulation, plain stores, no atomics: results are
 *   reproducible bit for bit.
 *   lora_conv_down:  h[(b, oy, ox)][c] (bf16 [B * Ho * Wo][r], contiguous) = scale * sum_{ky, kx, ci} x[nbr][ci] * f[c][ci][ky][kx];
 *                    x bf16 [B * H * W][C] with row stride ldx (hijacks.py:159 with a Conv2d lora_down).
 *   lora_conv_dx:    dx[(b, iy, ix)][ci] (+)= sum over the taps with (iy + 1 - ky) % stride == 0 and (ix + 1 - kx) % stride == 0 whose
 *                    output pixel exists, and over c, of dh[(b, (iy + 1 - ky) / stride, (ix + 1 - kx) / stride)][c] * f[c][ci][ky][kx];
 *                    dh bf16 [B * Ho * Wo][r] contiguous, dx bf16 [B * H * W][C] with row stride lddx.  accumulate == 0: plain
 *                    store; != 0: one read-modify-write pass (the base convolution's dX).  Every element has one producer lane.
 *   lora_conv_wgrad: out[c][ci][ky][kx] (+)= scale * sum_m dh[m][c] * x[nbr(m, ky, kx)][ci]; out f32 [r][C][3][3] (the layout of
 *                    lora_down.weight, written directly).  The reduction over the B * Ho * Wo rows is cut into row splits whose
 *                    f32 partial sums go to `workspace` (>= cfhip_lora_conv_wgrad_workspace(...) bytes) and are added in split
 *                    order by a second kernel.
 * ------------------------------------------------------------------------------------------ */
int cfhip_lora_conv_down(const void* x, const void* f, void* h, int B, int H, int W, int C, int r, int stride, int64_t ldx,
                         float scale, void* stream);
int cfhip_lora_conv_dx(const void* dh, const void* f, void* dx, int B, int H, int W, int C, int r, int stride, int64_t lddx,
                       int accumulate, void* stream);
size_t cfhip_lora_conv_wgrad_workspace(int B, int H, int W, int C, int r, int stride);
int cfhip_lora_conv_wgrad(const void* dh, const void* x, float* out, int B, int H, int W, int C, int r, int stride, int64_t ldx,
                          int accumulate, float scale, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * A16  tabular encoder (ml_encoder.Encoder.forward, modules/core/ml_encoder.py:171-209, + CommonMLModel.encode,
 *      models/ml/common.py:67-87) as one gather: out[b] = [numerical columns | one-hot blocks | embedding rows].
 *   plan: Fo entries of 6 int32 {src column, kind (0 copy / 1 one-hot / 2 embedding), payload (class id / table
 *     column), table id, dim (number of categories), table row pitch}, built by the host once per encoder.
 *   Categorical value v -> index: v >= dim -> 0 (the reference's out-of-bound imputation), else (int64)v
 *     (truncation, `.to(torch.long)`).  Integer index work: one-hot block and gathered rows are bit-exact.
 *   tables / dtables: device arrays of f32 base pointers, one per embedding column (`embeddings.<col>.weights`,
 *     [dim][pitch]); a NULL dtables entry skips that table's gradient.
 *   indices: int64 [B][K] of the K categorical columns (EncodingResult.indices).
 *   bwd: numerical outputs -> dx[b][src] (dx may be NULL), embedding outputs -> f32 atomic scatter-add into dtables
 *     (caller zeroes / owns them); one-hot outputs carry no gradient.
 * ------------------------------------------------------------------------------------------ */
int cfhip_ml_encode_fwd(const float* x, int64_t B, int F, int64_t x_row_stride, const int32_t* plan, int Fo,
                        const void* const* tables, float* out, void* stream);
int cfhip_ml_encode_indices(const float* x, int64_t B, int64_t x_row_stride, const int32_t* cols, const int32_t* dims,
                            int K, int64_t* indices, void* stream);
int cfhip_ml_encode_bwd(const float* dout, const float* x, int64_t B, int F, int64_t x_row_stride, const int32_t* plan,
                        int Fo, void* const* dtables, float* dx, void* stream);


/* ------------------------------------------------------------------------------------------
 * C1 / C2 / C3  collectives of the data-parallel exchange over RCCL / xGMI.  Replace what
 *   `accelerator.prepare` -> torch DDP would have done behind trainer.py:268-272 (gradient all-reduce, C1; the DDP
 *   constructor's parameter broadcast, C3) and add the embedding all-gather / reduce-scatter of a contrastive step (C2).
 *   One communicator per process (one process per GPU).  RCCL is reached with dlopen (the copy the process already
 *   holds — torch's — is preferred), so libcfhip.so has no link-time RCCL dependency.
 *   unique_id: rank 0 fills 128 bytes (ncclGetUniqueId); the caller ships them to the other ranks (any host channel:
 *     the launcher's TCP store, a file).  init: collective over all ranks; the CURRENT HIP device is the rank's GPU.
 *   Every collective is in-stream on `stream` (caller's comm stream), never synchronises the host.
 *   dtype: 0 = f32, 1 = bf16.  allreduce / broadcast are in place; allgather / reduce_scatter take `count_per_rank`
 *     elements per rank (recv of allgather / send of reduce_scatter hold world * count_per_rank).  Reductions are sums:
 *     the 1 / W of gradient averaging is the optimizer's grad_scale.
 * ------------------------------------------------------------------------------------------ */
int cfhip_comm_unique_id(void* out128);
int cfhip_comm_init(int rank, int world, const void* uid128, void** comm);
int cfhip_comm_destroy(void* comm);
/* ncclCommCount / ncclCommUserRank of the communicator: what RCCL reports, for the benchmark's evidence line (`rank` may be NULL) */
int cfhip_comm_count(void* comm, int* world, int* rank);
int cfhip_comm_allreduce(void* comm, void* buf, size_t count, int dtype, void* stream);
int cfhip_comm_allgather(void* comm, const void* send, void* recv, size_t count_per_rank, int dtype, void* stream);
int cfhip_comm_reduce_scatter(void* comm, const void* send, void* recv, size_t count_per_rank, int dtype, void* stream);
int cfhip_comm_broadcast(void* comm, void* buf, size_t count, int dtype, int root, void* stream);

/* ------------------------------------------------------------------------------------------
 * Grouped convolution (groups > 1, depthwise included): F.conv2d(net, w, bias, stride, padding, dilation, groups) reached
 * from Conv2d.forward (modules/core/convs/basic.py:160-177) and its two backward halves.  An option outside the named
 * benchmark configurations: direct kernels (one thread per output / input element, one workgroup per filter plane for the
 * weight gradient), fp32 accumulation, no atomics.  x / y / dy / dx bf16 NCHW; w bf16 [Cout][Cin / groups][kh][kw];
 * bias, dw, bias_grad f32; kh * kw <= 49 for the weight gradient.
 * ------------------------------------------------------------------------------------------ */
int cfhip_conv2d_grouped_fwd(const void* x, const void* w, const float* bias, void* y, int B, int Cin, int H, int W, int Cout,
                             int kh, int kw, int stride, int pad, int dil, int groups, void* stream);
int cfhip_conv2d_grouped_bwd_input(const void* dy, const void* w, void* dx, int B, int Cin, int H, int W, int Cout, int kh,
                                   int kw, int stride, int pad, int dil, int groups, void* stream);
int cfhip_conv2d_grouped_bwd_weight(const void* dy, const void* x, float* dw, int accumulate, float* bias_grad,
                                    int bias_grad_accumulate, int B, int Cin, int H, int W, int Cout, int kh, int kw,
                                    int stride, int pad, int dil, int groups, void* stream);

/* ------------------------------------------------------------------------------------------
 * Head-only tail of a pre-norm block (csrc/head_tail.hip, csrc/gemm.hip): the last block of a stack whose output is read at token
 * 0 only (`net[:, 0]`, the head-token classifier) needs K and V of every row, but its projection, FF1 + GELU, FF2 and their dX
 * GEMMs for the B head rows alone.  Those rows are computed IN PLACE in the full-size [B * T, .] tensors of the block: a GEMM of
 * M = B rows whose A / C / aux leading dimensions are T rows long, under the tile configuration of the whole B * T-row launch —
 *   cfhip_gemm_bf16_rows: cfhip_gemm_bf16 (a_trans = 0, no split-K, no bias gradient) with the tile configuration picked as for
 *     `config_rows` >= M rows.  An output element is the same K-ordered accumulation whatever rows share its launch, so the M rows
 *     come out bit-identical to the same rows of the whole launch.
 * The rows the GEMMs skip must read as zero to the full-row launches that stay (LayerNorm, attention backward, the weight
 * gradients, whose reductions then add exact zeros in the order they always had) —
 *   cfhip_head_rows_zero: the first `cols` elements of `rows` rows, `row_stride` elements apart, := 0 (16-byte stores).
 * ------------------------------------------------------------------------------------------ */
int cfhip_gemm_bf16_rows(const void* A, const void* B, void* C, const float* bias, const void* aux_in, void* aux_out, int M, int N,
                         int K, int64_t lda, int64_t ldb, int64_t ldc, int b_trans, int epilogue, int out_dtype, int config_rows,
                         void* stream);
int cfhip_head_rows_zero(void* dst, int rows, int cols, int64_t row_stride, int elem_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * GRU / LSTM recurrence (csrc/rnn.hip): what nn.GRU / nn.LSTM (ml/rnn.py:13-17, the rnn_dict) do past the input projection in the
 * single-layer, batch_first cells that ml/rnn.py:53-80 (_init_rnn) builds and ml/rnn.py:82-85 (forward, `rnn(net, None)`) runs.
 *   cell: CFHIP_RNN_GRU (gates r, z, n; G = 3) or CFHIP_RNN_LSTM (gates i, f, g, o; G = 4), PyTorch's definitions and weight order.
 *   H % 8 == 0, 8 <= H <= CFHIP_RNN_MAX_HIDDEN; B, T >= 1.  One workgroup owns 16 batch rows for all T steps and loops over time
 *   inside the launch; workgroups never wait for each other.  Row (b, t) of every [B T, .] operand is row b * T + t.
 *   rnn_pack: w_hh f32 [G H, H] -> `packed`, cfhip_rnn_pack_workspace(cell, H) bytes (0 for a refused shape), 16-byte aligned: W_hh
 *     as bf16 in MFMA fragment order, once for the forward product h W_hh^T and once for the backward product dgh W_hh.
 *   rnn_fwd: gx f32 [B T, G H] (= x W_ih^T + b_ih), b_hh f32 [G H]; h0 / c0 f32 [B, H] or NULL (zero); y: the hidden sequence,
 *     row (b, t) = H floats at y + (b * T + t) * ldy (ldy >= H: one half of a bidirectional [B, T, 2 H] buffer); hT / cT f32 [B, H]
 *     or NULL (not wanted); reverse != 0: step s works on t = T - 1 - s.  Training saves (each NULL = not saved): gates f32
 *     [B T, 4 H] (GRU: r, z, n, h W_hn^T + b_hn; LSTM: i, f, g, o), cseq f32 [B T, H] (LSTM: c_t), hprev16 bf16 [B T, H] (the state
 *     each step STARTED from, as the matrix operand: the B operand of dW_hh = dgh^T hprev16).
 *     The state is carried in f32 and rounded to bf16 only as the MFMA operand; a step's arithmetic does not depend on its index
 *     in the launch (one launch of T steps == T chained launches of one step passing hT -> h0, cT -> c0, bit for bit).
 *   rnn_bwd: the same walk backwards.  dy: gradient of y, row stride lddy, or NULL (zero); dhT / dcT f32 [B, H] or NULL (zero):
 *     gradients of hT / cT; y, h0, c0, gates, cseq: what rnn_fwd read and wrote (y and h0 are read by the GRU only).  Writes
 *     dgx bf16 [B T, G H] (gradient of gx), dgh bf16 [B T, G H] (gradient of h W_hh^T + b_hh; GRU only: the LSTM's IS dgx, pass
 *     NULL), dh0 / dc0 f32 [B, H] or NULL (not wanted).  Chains like the forward (dh0 -> dhT, dc0 -> dcT).
 * ------------------------------------------------------------------------------------------ */
#define CFHIP_RNN_GRU 0
#define CFHIP_RNN_LSTM 1
#define CFHIP_RNN_MAX_HIDDEN 256
size_t cfhip_rnn_pack_workspace(int cell, int H);
int cfhip_rnn_pack(const float* w_hh, void* packed, size_t packed_bytes, int cell, int H, void* stream);
int cfhip_rnn_fwd(const float* gx, const void* packed, const float* b_hh, const float* h0, const float* c0, float* y, int64_t ldy,
                  float* hT, float* cT, float* gates, float* cseq, void* hprev16, int cell, int64_t B, int T, int H, int reverse,
                  void* stream);
int cfhip_rnn_bwd(const float* dy, int64_t lddy, const float* dhT, const float* dcT, const void* packed, const float* y, int64_t ldy,
                  const float* h0, const float* c0, const float* gates, const float* cseq, void* dgx, void* dgh, float* dh0,
                  float* dc0, int cell, int64_t B, int T, int H, int reverse, void* stream);

/* ------------------------------------------------------------------------------------------
 * PixelCNN sampling (csrc/pixelcnn.hip): PixelCNN.sample (cv/ar/pixel_cnn.py:142-165), which runs img_size^2 full forwards
 * (pixel_cnn.py:136-140) through the masked convolutions of pixel_cnn.py:20-65 and draws one pixel from each, as ONE launch that
 * walks the pixels first_pixel .. last_pixel - 1 in raster order and computes one output column per layer and pixel (the eval-mode
 * net is causal).  One workgroup owns 16 batch rows for the whole launch; workgroups never wait for each other.
 *   codes int64 [B][1][H][W]: written at the launch's pixels (forced == 0) or read there (forced != 0: teacher forcing; every code
 *     must be inside [0, K): the CALLER checks).  label_row int32 [B]: the row of in_table each sample uses (< U, the caller checks).
 *   in_table bf16 [U][K][Cin0]: the input of the first masked layer for each code (to_blocks + channel padding of that code);
 *     Cin0 == 1 or Cin0 == C.  in0 bf16 [B][H][W][Cin0] and act bf16 [L][B][H][W][C]: the sampler's state, written at the launch's
 *     pixels and read at earlier ones; a launch with first_pixel > 0 continues the state an earlier launch left.
 *   packs: per layer the live taps (T = 24 for layer 0, mask "A"; 25 after, mask "B") of the filter as bf16 in MFMA fragment order,
 *     K index t Cin + c over the row-major taps t < T, zero-padded to a multiple of 32 (layer 0 first, then L - 1 packs of 25 C);
 *     scale, shift f32 [L][C]: BatchNorm's eval affine (1, 0 without a norm), applied in f32 before LeakyReLU(0.2).
 *   head_pack bf16 [ceil(K / 16)][C / 32][64 lanes][8], head_bias f32 [K]: the 1x1 head.
 *   logits f32: [B][H][W][K] when logits_per_pixel != 0 (kept for the caller), else a [B][K] scratch.
 *   The draw of pixel (b, i, j): word e % 4 of Philox4x32-10 counter offset + e / 4 under `seed`, e = (b H + i) W + j,
 *     u = (w >> 8) 2^-24, the smallest k whose running sum of exp(l - max) exceeds u * total (csrc/pixelcnn.hip states the f32 order).
 *   C % 32 == 0, 32 <= C <= CFHIP_PIXELCNN_MAX_CHANNELS; 2 <= K <= CFHIP_PIXELCNN_MAX_CODES; L >= 1.
 * ------------------------------------------------------------------------------------------ */
#define CFHIP_PIXELCNN_MAX_CHANNELS 256
#define CFHIP_PIXELCNN_MAX_CODES 1024
int cfhip_pixelcnn_sample(void* codes, const int* label_row, const void* in_table, void* in0, void* act, const void* packs,
                          const float* scale, const float* shift, const void* head_pack, const float* head_bias, float* logits,
                          int logits_per_pixel, int64_t B, int H, int W, int C, int Cin0, int L, int K, int first_pixel,
                          int last_pixel, int forced, uint64_t seed, uint64_t offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * Masked 7x7 convolution on the live taps only (csrc/conv_masked.hip): MaskedConv2d.forward (cv/ar/pixel_cnn.py:20-65; stride 1,
 * padding 3, as PixelCNN builds it at pixel_cnn.py:90-104 and runs it at pixel_cnn.py:136-140) and its two backward halves, without
 * the [B H W, 49 Cin] im2row matrix and without multiplying the 24 / 25 masked taps.  taps = 24 (mask "A") or 25 (mask "B"): the
 * first `taps` row-major positions of the 7x7 window.  Channels are multiples of 32 on both sides.
 *   conv_masked_pack: w f32 [Cout][Cin][7][7] -> bf16 [Cout][taps Cin] (k = t Cin + c; the forward's filters) or, transposed != 0,
 *     [Cin][taps Cout] (k = t Cout + n; the input gradient's).  Masked taps are never read.
 *   conv_masked_bf16: y[B][H][W][Co] = conv of x bf16 NHWC rows [B][H][W][Ci] with pack [Co][taps Ci] (+ bias f32 [Co] or NULL), bf16
 *     out.  mirror == 0: the forward (taps reach 3 rows up and 3 columns either side); mirror != 0: the same kernel on the mirrored
 *     tap set (3 rows down): the input gradient, x = dy rows, pack = the transposed one, Ci = Cout, Co = Cin.  f32 accumulation in a
 *     fixed order, no atomics.
 *   conv_masked_gather: rows [row0, row0 + nrows) of G[B H W][taps Ci], G[row][t Ci + c] = x[b][i + t / 7 - 3][j + t % 7 - 3][c]
 *     (zero outside the image): the operand of the weight gradient dy_rows^T G, in row chunks of a bounded workspace.
 * ------------------------------------------------------------------------------------------ */
int cfhip_conv_masked_pack(const float* w, void* pack, int Cout, int Cin, int taps, int transposed, void* stream);
int cfhip_conv_masked_bf16(const void* x, const void* pack, const float* bias, void* y, int B, int H, int W, int Ci, int Co, int taps,
                           int mirror, void* stream);
int cfhip_conv_masked_gather(const void* x, void* out, int64_t row0, int64_t nrows, int B, int H, int W, int Ci, int taps, void* stream);

/* ------------------------------------------------------------------------------------------
 * NBM, the neural basis model (csrc/nbm.hip): the per-basis MLPs that NBMBlock (ml/nbm.py:54-120) runs as grouped
 * nn.Conv1d(k = 1, groups = NB) layers (SeparableMapping, ml/nbm.py:18-51) over [B, NB H, D] tensors, and NBM's featurizer
 * Conv1d(D NB, D, 1, groups = D) (ml/nbm.py:168-174, applied at ml/nbm.py:189-194).
 *   Rows m = b D + d (M = B D < 2^31 - 1), NB bases, hidden width H (H % 8 == 0, 8 <= H <= CFHIP_NBM_MAX_HIDDEN), 1 <= order <=
 *   CFHIP_NBM_MAX_ORDER.  Per basis g: w1 f32 [NB][H][order], b1 [NB][H], W2 [NB][H][H], b2 [NB][H], w3 [NB][H], b3 [NB] (the
 *   conv weights of ml/nbm.py:36 seen as matrices).  idx int32 [D][order]: feature columns, every one inside the row of x.
 *   u[m][j] = x[b ldx + idx[d][j]];  h1 = relu(u w1^T + b1);  h2 = relu(h1 W2^T + b2);  bases[m][g] = h2 . w3 + b3.
 *   nbm_pack: W2 -> `packed`, cfhip_nbm_pack_workspace(NB, H) bytes (0 for a refused shape), 16-byte aligned: bf16 in MFMA fragment
 *     order, once for h1 W2^T and once, transposed, for the backward product dpre2 W2.
 *   nbm_bases_fwd: one launch for all bases and rows -> bases f32 [M][NB].  Layer 1 in f32 from the f32 features; h1 enters the
 *     products as TWO bf16 words, hi = bf16(h1) and lo = bf16(h1 - hi) (two MFMAs per 32 k; hi + lo = h1 to 2^-17); W2 as one
 *     bf16 word; f32 accumulation.  csrc/nbm.hip states the operation order.
 *   nbm_bases_bwd: saves nothing, recomputes from x, idx and the pack.  dbases f32 [M][NB] -> dw1, db1, dw2, db2, dw3, db3 (the
 *     parameters' shapes) and dx f32 [B][F] (written, never accumulated; a feature in several tuples or twice in one receives the
 *     sum).  A NULL destination is frozen: its sum is not reduced.  `accumulate`: bit 0 dw1, 1 db1, 2 dw2, 3 db2, 4 dw3, 5 db3 --
 *     set = add to the destination, clear = overwrite.  Sums over rows go through per-workgroup partials in `workspace`
 *     (cfhip_nbm_bases_bwd_workspace bytes, never 0 for an accepted shape, 16-byte aligned) and a fixed-order reduce: no
 *     floating-point atomics, two identical calls are bit-identical.  Neither pass touches a buffer of M NB H elements.
 *   nbm_featurize_fwd: feat[b][d] = sum_g bases[b][d][g] wf[d][g] + bf[d] (one f32 fma chain over g, then the bias).
 *   nbm_featurize_bwd: dfeat f32 [B][D] -> dbases [B][D][NB], dwf [D][NB] (needs bases), dbf [D]; NULL = not wanted;
 *     `accumulate`: bit 0 dwf, bit 1 dbf; sums over b in a fixed order through cfhip_nbm_featurize_bwd_workspace bytes.
 * ------------------------------------------------------------------------------------------ */
#define CFHIP_NBM_MAX_HIDDEN 256
#define CFHIP_NBM_MAX_ORDER 4
#define CFHIP_NBM_MAX_BASES 65536
size_t cfhip_nbm_pack_workspace(int NB, int H);
int cfhip_nbm_pack(const float* w2, void* packed, size_t packed_bytes, int NB, int H, void* stream);
int cfhip_nbm_bases_fwd(const float* x, int64_t ldx, const int* idx, const float* w1, const float* b1, const void* packed,
                        const float* b2, const float* w3, const float* b3, float* bases, int64_t B, int D, int NB, int H, int order,
                        void* stream);
size_t cfhip_nbm_bases_bwd_workspace(int64_t M, int NB, int H, int order, int want_dx);
int cfhip_nbm_bases_bwd(const float* dbases, const float* x, int64_t ldx, const int* idx, const float* w1, const float* b1,
                        const void* packed, const float* b2, const float* w3, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                        float* db3, float* dx, int accumulate, void* workspace, size_t workspace_bytes, int64_t B, int D, int F, int NB,
                        int H, int order, void* stream);
int cfhip_nbm_featurize_fwd(const float* bases, const float* wf, const float* bf, float* feat, int64_t B, int D, int NB, void* stream);
size_t cfhip_nbm_featurize_bwd_workspace(int64_t B, int D, int NB);
int cfhip_nbm_featurize_bwd(const float* dfeat, const float* bases, const float* wf, float* dbases, float* dwf, float* dbf,
                            int accumulate, void* workspace, size_t workspace_bytes, int64_t B, int D, int NB, void* stream);

/* ------------------------------------------------------------------------------------------
 * RWKV mixers (csrc/rwkv.hip): the time shift and mixes, the WKV term and the gates of RWKVTokenMixer
 * (mixed_stacks/token_mixers.py:107-206) and RWKVChannelMixer (mixed_stacks/channel_mixers.py:69-113).  The four / three Linear
 * layers are the GEMMs of csrc/gemm.hip.  No floating-point atomics: every sum over rows goes through per-workgroup partials in a
 * caller-owned workspace and a fixed-order reduce, two identical calls are bit-identical.
 *   time_mix_fwd: replaces token_mixers.py:179-182 / channel_mixers.py:107-109.  x [B][T][C] (f32 when x_f32 != 0, else bf16), mixes
 *     f32 [C]; out_j[b][t][c] = bf16(x[t] m_j + x[t-1] (1 - m_j)) in f32 (one subtraction, one product, one fma), x[-1] = 0 for
 *     every sample.  mv == NULL (and out_v == NULL): the two mixes of the channel mixer.
 *   time_mix_bwd: d_j [B][T][C] (f32 when d_f32 != 0, else bf16: the input gradients of the GEMMs) ->
 *     dx[t] = sum_j (d_j[t] m_j + d_j[t+1] (1 - m_j)) (the t+1 term absent at t = T-1), in x's dtype, NULL = not wanted;
 *     dm_j[c] = sum_{b,t} d_j[t] (x[t] - x[t-1]), NULL = frozen (neither computed nor reduced).
 *     `accumulate`: bit 0 dmk, 1 dmv, 2 dmr.  cfhip_rwkv_time_mix_bwd_workspace bytes (never 0 for an accepted shape).
 *   wkv_fwd: replaces token_mixers.py:184-203 (the two T-tap grouped conv1d calls, their pads and transposes, the sigmoid gate).
 *     k, v, r f32 [B][T][L], info_decay f32 [L]; lam = exp(-exp(info_decay)); e = exp(k); a[t] = lam a[t-1] + e[t];
 *     n[t] = e[t] v[t] / (a[t] + 1e-6); b[t] = lam b[t-1] + n[t]; y = bf16(sigmoid(r) b).  a, b f32 [B][T][L]: saved for the
 *     backward, both NULL = nothing saved.  Channels across lanes, time in chunks of CFHIP_RWKV_CHUNK steps over the waves of a
 *     workgroup; a chunk's result is lam^(t - t0 + 1) * carry + local, the carries pass through LDS chunk by chunk.  `waves`: chunks
 *     per pass of a workgroup, 1 .. CFHIP_RWKV_MAX_WAVES, 0 = chosen from the shape; the result's bits do not depend on it.
 *   wkv_bwd: dy (f32 when dy_f32 != 0, else bf16) -> dk, dv, dr bf16 [B][T][L] by the reverse recurrences (csrc/rwkv.hip states them), d_decay f32 [L] (NULL =
 *     frozen, `accumulate` != 0 adds) through cfhip_rwkv_wkv_bwd_workspace bytes of per-workgroup partials.
 *   relu2_fwd / relu2_bwd: replace channel_mixers.py:111.  out = bf16(relu(h)^2); dh = bf16(2 relu(h) d), d and h f32 or bf16.
 *   gate_fwd / gate_bwd: replace channel_mixers.py:113.  out = sigmoid(r) kv (+ residual, f32 or bf16, NULL = none), r and kv f32,
 *     out f32 or bf16; dr = bf16(d kv s (1 - s)), dkv = bf16(d s), d f32 or bf16.
 *   1 <= T, C, L; B T below 2^31; B T C, B T L and n at most 2^38; the scan takes B <= 65535 samples per launch.
 * ------------------------------------------------------------------------------------------ */
#define CFHIP_RWKV_CHUNK 8
#define CFHIP_RWKV_MAX_WAVES 16
int cfhip_rwkv_time_mix_fwd(const void* x, int x_f32, const float* mk, const float* mv, const float* mr, void* out_k, void* out_v,
                            void* out_r, int64_t B, int T, int C, void* stream);
size_t cfhip_rwkv_time_mix_bwd_workspace(int64_t B, int T, int C);
int cfhip_rwkv_time_mix_bwd(const void* dk, const void* dv, const void* dr, int d_f32, const void* x, int x_f32, const float* mk,
                            const float* mv, const float* mr, void* dx, float* dmk, float* dmv, float* dmr, int accumulate, void* workspace,
                            size_t workspace_bytes, int64_t B, int T, int C, void* stream);
int cfhip_rwkv_wkv_fwd(const float* k, const float* v, const float* r, const float* info_decay, void* y, float* a, float* b, int64_t B,
                       int T, int L, int waves, void* stream);
size_t cfhip_rwkv_wkv_bwd_workspace(int64_t B, int L);
int cfhip_rwkv_wkv_bwd(const void* dy, int dy_f32, const float* k, const float* v, const float* r, const float* info_decay,
                       const float* a, const float* b, void* dk, void* dv, void* dr, float* d_decay, int accumulate, void* workspace,
                       size_t workspace_bytes, int64_t B, int T, int L, int waves, void* stream);
int cfhip_rwkv_relu2_fwd(const void* h, int h_f32, void* out, int64_t n, void* stream);
int cfhip_rwkv_relu2_bwd(const void* d, int d_f32, const void* h, int h_f32, void* dh, int64_t n, void* stream);
int cfhip_rwkv_gate_fwd(const float* r, const float* kv, const void* residual, int residual_f32, void* out, int out_f32, int64_t n,
                        void* stream);
int cfhip_rwkv_gate_bwd(const void* d, int d_f32, const float* r, const float* kv, void* dr, void* dkv, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Siren, the sine-activated coordinate MLP (csrc/siren.hip): the layer stack of Siren.forward (implicit/siren.py:156-187), i.e.
 * num_layers times SirenLayer (siren.py:67-70: F.linear, then the sine) times the sample's modulation (siren.py:185-186), then the
 * head (siren.py:187), and the stand-alone sine activation that SirenLayer builds (siren.py:65).
 *   Rows r = b N + n, M = B N below 2^31 - 1, sample b = r / N; latent a multiple of 32 in 32 .. CFHIP_SIREN_MAX_LATENT,
 *   1 <= in_dim <= CFHIP_SIREN_MAX_IN, 1 <= out_dim <= CFHIP_SIREN_MAX_OUT, num_layers >= 1.  x f32 [M][in_dim], or with x_shared
 *   != 0 the grid buffer of make_grid (siren.py:21-24) f32 [N][in_dim] that every sample shares: the repeat of siren.py:183 is never
 *   materialised.  w0 f32 [latent][in_dim]; bias f32 [num_layers latent + out_dim] (the layers' biases, then the head's) or NULL
 *   (bias=False); mods f32 [num_layers][B][latent].
 *   siren_pack: W f32 [rows][K] (a hidden layer's weight, rows = K = latent, or the head's, rows = out_dim) -> bf16 in MFMA fragment
 *     order for the forward and, with_transposed != 0, for the backward product after it; cfhip_siren_pack_workspace(rows, K,
 *     with_transposed) bytes (0 for a refused shape), 16-byte aligned.  `packed` of the other entries: the num_layers - 1 hidden
 *     packs in layer order, all with the transposed part (siren_bwd; siren_fwd with packed_transposed != 0) or all without, then the
 *     head's forward pack alone (the backward reads the head's f32 weight).
 *   siren_fwd: ONE launch for all layers and the head -> out f32 [M][out_dim].  Layer 0 in f32 from the f32 coordinates with the
 *     accurate sine; hidden layers and the head on bf16 MFMA with f32 accumulation, the activation tile in LDS.  save_sin / save_cos:
 *     bf16 [num_layers][M][latent] for the backward, both NULL = nothing saved and no [M][latent] tensor written at all.
 *   siren_bwd: dy f32 [M][out_dim] -> dx f32 [M][in_dim] (NULL = not wanted), dpre bf16 [num_layers - 1][M][latent] and hprev bf16
 *     [num_layers - 1][M][latent] (the operands of the caller's tn GEMM for the hidden weights' gradients: dW_l = dpre[l - 1]^T
 *     hprev[l - 1]; NULL = not wanted; both, like the saved words, 16-byte aligned: they move as 16-byte rows), and per-tile partial sums in cfhip_siren_bwd_workspace bytes (never 0 for an accepted shape,
 *     16-byte aligned).  head_w: the head's f32 weight [out_dim][latent].
 *   siren_reduce: one destination from the workspace siren_bwd filled, in a fixed order: kind CFHIP_SIREN_DB (the bias of `layer`,
 *     [latent]), _DW0 ([latent][in_dim]), _DWHEAD ([out_dim][latent]), _DBHEAD ([out_dim]), _DMODS ([num_layers][B][latent]).  A
 *     frozen parameter is a call that is not made.  No floating-point atomics; two identical calls are bit-identical.
 *   sine_fwd / sine_bwd: y = sin(w x); dx = dy w cos(w x) on n f32 elements (activations.py: `sine`).
 * ------------------------------------------------------------------------------------------ */
#define CFHIP_SIREN_MAX_LATENT 256
#define CFHIP_SIREN_MAX_IN 8
#define CFHIP_SIREN_MAX_OUT 16
#define CFHIP_SIREN_DB 0
#define CFHIP_SIREN_DW0 1
#define CFHIP_SIREN_DWHEAD 2
#define CFHIP_SIREN_DBHEAD 3
#define CFHIP_SIREN_DMODS 4
size_t cfhip_siren_pack_workspace(int rows, int K, int with_transposed);
int cfhip_siren_pack(const float* w, void* packed, size_t packed_bytes, int rows, int K, int with_transposed, void* stream);
int cfhip_siren_fwd(const float* x, int x_shared, const float* w0, const void* packed, int packed_transposed, const float* bias,
                    const float* mods, float* out, void* save_sin, void* save_cos, int64_t B, int64_t N, int in_dim, int latent, int out_dim, int num_layers,
                    float w_first, float w_hidden, void* stream);
size_t cfhip_siren_bwd_workspace(int64_t B, int64_t N, int in_dim, int latent, int out_dim, int num_layers);
int cfhip_siren_bwd(const float* dy, const float* x, int x_shared, const float* w0, const void* packed, const float* head_w,
                    const float* mods, const void* save_sin, const void* save_cos, float* dx, void* dpre, void* hprev, void* workspace,
                    size_t workspace_bytes, int64_t B, int64_t N, int in_dim, int latent, int out_dim, int num_layers, float w_first,
                    float w_hidden, void* stream);
int cfhip_siren_reduce(const void* workspace, size_t workspace_bytes, int kind, int layer, float* dest, int accumulate, int64_t B,
                       int64_t N, int in_dim, int latent, int out_dim, int num_layers, void* stream);
int cfhip_sine_fwd(const float* x, float* y, int64_t n, float w, void* stream);
int cfhip_sine_bwd(const float* dy, const float* x, float* dx, int64_t n, float w, void* stream);
/* the ReLU of Modulator (siren.py:80-83) on f32 rows: y = max(x, 0); dx = y > 0 ? dy : 0 from the saved output.  The modulator
 * runs in f32 (its Linear on cfhip_sgemm_f32): in bf16 a pre-activation near zero flips its mask, and with B rows only a few flips
 * put the modulator's gradients at the reference's own bf16-autocast distance. */
int cfhip_relu_f32_fwd(const float* x, float* y, int64_t n, void* stream);
int cfhip_relu_f32_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFHIP_H */
