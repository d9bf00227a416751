/*
 * deepmerge_hip.h -- C-ABI of libdeepmerge_hip.so, the MI355X (gfx950) kernels behind the
 * DeepMerge pair-encoder hot path.
 *
 * The reference (lvxianwei/DeepMerge) has NO native/FFI boundary: the path sits behind plain
 * Python torch.nn.Module classes that call stock torch ops.  Each entry point below therefore
 * cites the reference *Python* statement(s) whose arithmetic it replaces (file:line relative to
 * the reference tree); INTEGRATION.md shows the ctypes binding and the module-level drop-in.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (torch storage); the library
 *     never allocates, frees or retains memory and never synchronises the device;
 *   - every call enqueues on the caller's `stream` (hipStream_t passed as void*; NULL = default);
 *   - return value: 0 on success, negative DmStatus otherwise; dm_last_error() gives a
 *     thread-local message; no C++ exception crosses the boundary;
 *   - `dtype` arguments take DmDtype; "T" below means the activation type of the numerics mode:
 *     DM_BF16 (throughput mode: bf16 operands, fp32 accumulate) or DM_F32 (parity mode: fp32
 *     operands on the f32-input MFMA, bit-equivalent to an fmaf chain);
 *   - all matrices are row-major with an explicit leading dimension in ELEMENTS.
 */
#ifndef DEEPMERGE_HIP_H
#define DEEPMERGE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { DM_F32 = 0, DM_BF16 = 1,
               DM_BF16_PAIR = 2,     /* ABI 4, DmGemmArgs.c_dtype only: C is written as a hi / lo plane pair (see c_plane) */
               DM_F64 = 3            /* dm_pairwise_distance only */
} DmDtype;

typedef enum {
  DM_OK = 0,
  DM_ERR_BAD_SHAPE = -1,
  DM_ERR_BAD_DTYPE = -2,
  DM_ERR_BAD_ALIGN = -3,
  DM_ERR_WORKSPACE = -4,
  DM_ERR_HIP = -5,
  DM_ERR_UNSUPPORTED = -6
} DmStatus;

/* ---- library ------------------------------------------------------------------------- */
int dm_abi_version(void);   /* 2: dm_patch_pyramid / dm_patch_pyramid_cols take a resize rule; 3: table-reading and split-bf16 attention entry points, dm_split_bf16_colsum (round 3);
                             * 4: DmGemmArgs.k_fold / a_fold / b_fold, dm_split_bf16_planes (round 4); 5: dm_pair_batch_gather (round 5); 6: dm_gemm_grouped (round 5);
                             * 7: dm_gemm_grouped(args, n, stream) without a group workspace, its workspace query removed;
                             * additive in 6: dm_pairwise_distance, dm_pair_epoch_draw, dm_contrastive_terms, dm_pair_eval_summary;
                             * additive in 7: dm_region_merge_cost, dm_pixel_regions, dm_pair_batch_gather_oriented, dm_pair_epoch_orient,
                             *   dm_pair_batch_gather_augmented, dm_pair_epoch_radiometric, dm_pair_epoch_select, dm_pair_epoch_draw_src,
                             *   dm_pair_epoch_orient_src, dm_pair_epoch_radiometric_src */
const char *dm_last_error(void);
/* Name of the code object architecture the library was built for ("gfx950"). */
const char *dm_arch(void);

/* ---- GEMM family (MFMA, LDS-staged 128x128 tiles) ---------------------------------------
 * Replaces every nn.Linear / k=stride Conv2d / k=1 Conv1d on the path and their autograd:
 *   qkv, proj        nets/ShfitScaleFormer.py:119, :134        (vit_model.py:119, :133)
 *   fc1, fc2         nets/ShfitScaleFormer.py:53, :56          (vit_model.py:152-156)
 *   PatchEmbed.proj  nets/ShfitScaleFormer.py:35               (after dm_patchify)
 *   FeatureEmbed     nets/ShfitScaleFormer.py:76-79, final Linear :948 / :967
 * layout: DM_NT  C[m,n] = sum_k A[m,k] * B[n,k]   (forward  y = x W^T,  W = [out,in])
 *         DM_NN  C[m,n] = sum_k A[m,k] * B[k,n]   (dgrad    dx = dy W)
 *         DM_TN  C[m,n] = sum_k A[k,m] * B[k,n]   (wgrad    dW = dy^T x)
 * epilogue, applied in this order on the fp32 accumulator v of element (m,n):
 *   v += bias[n]                     if bias != NULL
 *   aux[m,n] = v (as aux_dtype)      if epilogue == DM_EPI_GELU     (pre-activation saved for backward; aux may be NULL:
 *                                       inference, nothing saved)
 *   v  = gelu_erf(v)                 if epilogue == DM_EPI_GELU     (nn.GELU, erf form)
 *   v *= gelu_erf'(aux[m,n])         if epilogue == DM_EPI_DGELU    (backward through GELU)
 *   aux[m,n] = gelu_erf'(v); v = gelu_erf(v)   if epilogue == DM_EPI_GELU_GRAD  (the derivative is saved instead of the
 *                                       pre-activation: same bytes, and the backward epilogue becomes one multiply)
 *   v *= aux[m,n]                    if epilogue == DM_EPI_MUL      (backward through GELU with the saved derivative)
 *   v += residual[m,n]               if residual != NULL (fp32)
 *   v += C_old[m,n]                  if accumulate (C must be fp32; not with DM_EPI_DGELU / DM_EPI_MUL: DM_ERR_UNSUPPORTED)
 *   C[m,n] = v (as c_dtype)
 * split_k > 1 (DM_TN only): the contraction is cut into split_k slices whose fp32 partial tiles
 * go to `workspace` ([split_k, M, N] floats) and are summed deterministically by a second
 * kernel that applies the epilogue.  split_k == 0 lets the library choose.
 */
typedef enum { DM_NT = 0, DM_NN = 1, DM_TN = 2 } DmGemmLayout;
typedef enum { DM_EPI_NONE = 0, DM_EPI_GELU = 1, DM_EPI_DGELU = 2, DM_EPI_GELU_GRAD = 3, DM_EPI_MUL = 4 } DmEpilogue;

typedef struct {
  int32_t layout;        /* DmGemmLayout */
  int32_t ab_dtype;      /* DmDtype of A and B */
  int32_t c_dtype;       /* DmDtype of C */
  int32_t aux_dtype;     /* DmDtype of aux */
  int32_t M, N, K;
  int32_t epilogue;      /* DmEpilogue */
  int32_t accumulate;    /* 0/1 */
  int32_t split_k;       /* 0 = auto, 1 = none */
  const void *A; int64_t lda;
  const void *B; int64_t ldb;
  void *C; int64_t ldc;
  const float *bias;                     /* [N] or NULL */
  const float *residual; int64_t ldr;    /* [M,N] fp32 or NULL */
  void *aux; int64_t ldaux;              /* see epilogue */
  /* Optional two-level row addressing of C / residual / aux: row m lives at
   * (m / rows_per_group) * group_stride + (m % rows_per_group) * ld.  rows_per_group == 0: plain.
   * Used to write each scale's 64 patch tokens into its slice of the token cube (torch.cat at
   * nets/ShfitScaleFormer.py:877). */
  int32_t rows_per_group; int64_t group_stride;
  void *workspace; int64_t workspace_bytes;
  /* DM_TN only, optional: colsum_a[m] (+)= sum_k A[k,m], fp32 [M] -- the bias gradient that goes with a weight gradient
   * dW = dy^T x (autograd of nn.Linear's bias: column sums of dy).  On the 256x256 wgrad pipeline it costs a few extra
   * MFMAs against a ones fragment instead of another pass over dy; otherwise dm_gemm runs the column-sum kernels itself.
   * Needs the workspace (dm_gemm_workspace_bytes covers it). */
  float *colsum_a; int32_t colsum_accumulate;
  /* ABI 4, optional: folded contraction for the "bf16x3" products on hi / lo PLANE PAIRS (dm_split_bf16_planes).  k_fold > 0:
   * K == 3 * k_fold, and the K segment s = 0, 1, 2 of A is the plain operand (same layout, same lda, contraction length k_fold)
   * that starts a_fold[s] ELEMENTS behind A -- {0, 0, plane} for the left operand (hi, hi, lo), {0, plane, 0} for the right one
   * (hi, lo, hi), plane = rows * ld of the plane pair.  Every tensor is then split ONCE, whatever side and layout its consumers
   * read it in, and the hi plane is fetched twice from the same addresses instead of being stored twice.
   * bf16 operands only; k_fold % 64 == 0; 0 <= offsets < 2^30.  With colsum_a (DM_TN) the sums are colsum(hi plane) +
   * colsum(lo plane) of A, fp32 -- the bias gradient to the accuracy of the folded product itself, NOT the exact fp32 column sum of
   * the unsplit tensor (the segment that re-reads the hi plane is skipped).  Shapes the folded kernels do not take return
   * DM_ERR_UNSUPPORTED; nothing falls back inside the library (a caller may split into dm_split_bf16 images and call again). */
  int32_t k_fold;
  int64_t a_fold[3], b_fold[3];
  /* ABI 4: c_dtype == DM_BF16_PAIR writes the result as the hi / lo plane pair a later folded product reads (the split pass of
   * that tensor disappears): hi = bf16(v) at C[m * ldc + n], lo = bf16(v - hi) at C[c_plane + m * ldc + n], C a bf16 pointer, ldc and
   * c_plane in bf16 elements (multiples of 8).  Not with accumulate; NT / NN products on the MFMA path (DM_ERR_UNSUPPORTED otherwise). */
  int64_t c_plane;
} DmGemmArgs;

int dm_gemm(const DmGemmArgs *args, void *stream);
/* Bytes of workspace dm_gemm may use for these dimensions (upper bound over split_k choices). */
int64_t dm_gemm_workspace_bytes(int32_t layout, int32_t M, int32_t N, int32_t K);
/* ABI 6, three arguments since ABI 7: n INDEPENDENT products (no output overlaps another product's operands or output), results as n dm_gemm
 * calls in order -- weight gradients up to the order of the fp32 additions over K.  The four weight gradients of a transformer block (dW = dy^T x
 * for qkv / proj / fc1 / fc2: nets/ShfitScaleFormer.py:35, :119, :134 and vit_model.py:112-135, :160-176 under autograd) feed nothing else in the
 * block's backward pass.  Alone each has 12 .. 48 output tiles of 256 x 192: it either leaves most CUs idle or pays up to 16 K slices, a slab
 * round trip of as many partial gradients and a reduction launch.  Fast path: 2 .. 8 bf16 DM_TN products (plain operands or hi / lo plane pairs
 * through k_fold; fp32 C, no epilogue operands, split_k == 0, M % 256 == N % 192 == 0, K % 128 == 0) in ONE launch, in one of two forms:
 *   one-slice: contraction <= 12288, all tiles within one round of the CUs, the same `accumulate` for all: one K slice per tile, the gradient
 *   stored / accumulated in place (the form the training step uses: -3.0 % on the headline step);
 *   sliced: contraction > 12288, the same for all products, tiles x slices >= 0.85 of the CUs: the SAME K slices for every product, (product,
 *   tile, slice) per workgroup, partial tiles to each product's own workspace slab and its own reduction behind (the 12-tile proj gradient
 *   next to the qkv gradient: 5 slices on 240 workgroups instead of 16 + 7 on two launches; -1.1 % on the headline step).
 * colsum_a is produced by the same launch.  Every other group: the calls one after the other (same errors as dm_gemm) -- also when
 * DM_GEMM_GROUPED=0, DM_GEMM_W4=0 or DM_GEMM_W4_TN=0 is set or DM_GEMM_ROUTE names a member (A/B runs; DM_GEMM_GROUPED=2 / 4: the one-slice /
 * sliced form whenever legal).  Each args[i] carries its own workspace, as for dm_gemm; the group has none. */
int dm_gemm_grouped(const DmGemmArgs *args, int32_t n, void *stream);

/* ---- fused attention with 3-D relative-position bias -------------------------------------
 * Replaces nets/ShfitScaleFormer.py:119-133 (reshape/permute, q*scale, q@k^T, bias add, softmax,
 * attn@v, transpose/reshape) and vit_model.py:119-133 (bias == NULL; the scale 64^-0.5 = 2^-3 is
 * exact, so applying it before or after q@k^T is bit-identical).
 *   qkv   [B, N, 3, H, D]  T   (output of the qkv Linear).  D = 64 and N <= 256 run the MFMA kernels; any other head dim <= 128 /
 *                            N <= 4096 (ViT-H/14: D = 80, N = 257) a plain fp32 kernel family (no bias-table gradient there)
 *   bias  [H, N, N] fp32 or NULL  (dense, from dm_relpos_bias_gather)
 *   out   [B, N, H*D]      T
 *   lse   [B, H, N] fp32   row log-sum-exp of the biased scores (saved for backward)
 */
int dm_attention_fwd(const void *qkv, const float *bias, void *out, float *lse,
                     int32_t B, int32_t N, int32_t H, int32_t D, float scale, int32_t dtype, void *stream);
/* The same forward with the bias taken inside the kernel from relative_position_bias_table [n_bins, H] fp32 of a
 * (cube_s, cube_h, cube_w) token cube (tokens scale-major then row-major, index rule of nets/ShfitScaleFormer.py:139-156):
 * the dense [H,N,N] rows of dm_relpos_bias_gather are never formed.  dm_attention_relpos_inkernel returns 1 for the
 * shapes this takes (bf16, D = 64, cube (3|4, 8, 8), N = 64 cube_s, B*H >= 96) and 0 otherwise: for those, gather and
 * call dm_attention_fwd (dm_attention_fwd_relpos returns DM_ERR_UNSUPPORTED without launching anything).  Results equal dm_attention_fwd's
 * on the gathered bias up to fp32 rounding of bias / scale. */
int32_t dm_attention_relpos_inkernel(int32_t B, int32_t N, int32_t H, int32_t D, int32_t cube_s, int32_t cube_h,
                                     int32_t cube_w, int32_t dtype);
int dm_attention_fwd_relpos(const void *qkv, const float *table, int32_t cube_s, int32_t cube_h, int32_t cube_w,
                            void *out, float *lse, int32_t B, int32_t N, int32_t H, int32_t D, float scale,
                            int32_t dtype, void *stream);
/* Backward: dqkv [B,N,3,H,D] T (fully written).  If dbias_slab != NULL the gradient of the dense bias is written
 * too: dbias_slab[c][h][i][j] = sum over the samples of batch chunk c of dS[b,h,i,j], fp32, fully written,
 * dm_attention_bwd_batch_chunks(B,N,H) * H * N * N floats; fold it into the table's gradient with
 * dm_relpos_bias_reduce.  No atomics are used anywhere, so every output is run-to-run deterministic.
 * delta is a [B,H,N] fp32 scratch.  bias_t (optional) is the per-head transpose of bias, bias_t[h][key][q], which
 * lets the key-major kernel read the bias with coalesced vector loads; NULL falls back to strided reads of `bias`. */
int dm_attention_bwd(const void *qkv, const float *bias, const float *bias_t, const void *out, const void *dout,
                     const float *lse, void *dqkv, float *delta, float *dbias_slab, int32_t B, int32_t N, int32_t H,
                     int32_t D, float scale, int32_t dtype, void *stream);
/* dm_attention_bwd for the shapes dm_attention_relpos_inkernel takes: both passes form the bias from the table inside
 * the kernel, so bias / bias_t may be NULL (they are only read when the table kernels are switched off for A/B runs).
 * dbias_slab as for dm_attention_bwd (same chunk count, same layout, deterministic); its entries are sums of dS values
 * rounded to bf16 (the operand the dK product consumes), accumulated in fp32. */
int dm_attention_bwd_relpos(const void *qkv, const float *table, int32_t cube_s, int32_t cube_h, int32_t cube_w,
                            const float *bias, const float *bias_t, const void *out, const void *dout, const float *lse,
                            void *dqkv, float *delta, float *dbias_slab, int32_t B, int32_t N, int32_t H, int32_t D,
                            float scale, int32_t dtype, void *stream);
/* Attention of the "bf16x3" numerics mode: fp32 tensors, every product as a split-bf16 triple on the matrix pipe (hi.hi +
 * lo.hi + hi.lo into fp32: ~2^-17 relative per product, where the plain fp32 entry points above use fp32 FMA / fp32 MFMA
 * arithmetic at a fraction of the rate).  Replaces the same reference statements as dm_attention_fwd.  qkv_hi / qkv_lo:
 * caller-allocated bf16 tensors of qkv's shape, WRITTEN here (hi = bf16(x), lo = bf16(x - hi)) and kept by the caller for
 * the backward pass -- or, with qkv == NULL (ABI 4), READ here: the caller filled them (the qkv product with a DM_BF16_PAIR result).
 * table: NULL (no bias) or the relative-position table of a (cube_s, 8, 8) token cube as for
 * dm_attention_fwd_relpos.  dm_attention_split_ok returns 1 for the shapes taken (D = 64, 128 < N <= 256, cube (3|4, 8, 8)
 * when a table is given). */
int32_t dm_attention_split_ok(int32_t B, int32_t N, int32_t H, int32_t D, int32_t has_table, int32_t cube_s, int32_t cube_h,
                              int32_t cube_w);
int dm_attention_split_fwd(const float *qkv, void *qkv_hi, void *qkv_lo, const float *table, int32_t cube_s, int32_t cube_h,
                           int32_t cube_w, float *out, float *lse, int32_t B, int32_t N, int32_t H, int32_t D, float scale,
                           void *stream);
/* The same with the hi / lo PLANE PAIR of `out` written on the side (out_pair bf16 [2][B*N, H*64]; ABI 4): the output projection of the
 * "bf16x3" mode reads it as its folded left operand (DmGemmArgs.k_fold). */
int dm_attention_split_fwd_pair(const float *qkv, void *qkv_hi, void *qkv_lo, const float *table, int32_t cube_s, int32_t cube_h,
                                int32_t cube_w, float *out, void *out_pair, float *lse, int32_t B, int32_t N, int32_t H, int32_t D,
                                float scale, void *stream);
/* Backward of dm_attention_split_fwd: dqkv [B,N,3,H,64] fp32 fully written; qkv_hi / qkv_lo as the forward left them;
 * dout_hi / dout_lo: caller-allocated bf16 scratch of dout's shape (written here); delta [B,H,N] scratch; dbias_slab
 * (needs the table): dm_attention_split_bwd_chunks(B,N,H) x H x N x N floats, layout and reduction as for dm_attention_bwd. */
int32_t dm_attention_split_bwd_chunks(int32_t B, int32_t N, int32_t H);
int dm_attention_split_bwd(const void *qkv_hi, const void *qkv_lo, const float *table, int32_t cube_s, int32_t cube_h,
                           int32_t cube_w, const float *out, const float *dout, void *dout_hi, void *dout_lo,
                           const float *lse, float *dqkv, float *delta, float *dbias_slab, int32_t B, int32_t N,
                           int32_t H, int32_t D, float scale, void *stream);
/* The same with dqkv written as a hi / lo PLANE PAIR (dqkv_pair bf16 [2][B,N,3,H,64]; ABI 4) instead of fp32: the operand format of the
 * folded qkv weight / data gradient products (DmGemmArgs.k_fold), which then need no split pass. */
int dm_attention_split_bwd_pair(const void *qkv_hi, const void *qkv_lo, const float *table, int32_t cube_s, int32_t cube_h,
                                int32_t cube_w, const float *out, const float *dout, void *dout_hi, void *dout_lo,
                                const float *lse, void *dqkv_pair, float *delta, float *dbias_slab, int32_t B, int32_t N,
                                int32_t H, int32_t D, float scale, void *stream);
/* Number of batch chunks dm_attention_bwd uses for this problem size and dtype (first dimension of dbias_slab). */
int32_t dm_attention_bwd_batch_chunks(int32_t B, int32_t N, int32_t H, int32_t dtype);

/* relative_position_bias_table[index.view(-1)].view(N,N,H).permute(2,0,1)
 * (nets/ShfitScaleFormer.py:123-128): table [n_bins,H] fp32, index int32 [N,N] -> bias [H,N,N] and,
 * if bias_t != NULL, its per-head transpose bias_t[h][j][i] = bias[h][i][j]. */
int dm_relpos_bias_gather(const float *table, const int32_t *index, float *bias, float *bias_t,
                          int32_t N, int32_t H, int32_t n_bins, void *stream);
/* Autograd of that gather (the index_put the reference's autograd performs for table[index], :123-128):
 *   dtable[bin,h] (+)= sum_c sum_{(i,j): index[i,j] == bin} dbias_slab[c][h][i][j]
 * `positions` (int32, flat i*N+j, ascending within a bin) and `offsets` (int32 [n_bins+1]) are the CSR inverse of the
 * index: positions[offsets[bin] .. offsets[bin+1]) are the entries that read table row `bin`.  Fixed summation
 * order: deterministic.  The slab is scratch: its first chunk is overwritten with the sum over chunks. */
int dm_relpos_bias_reduce(float *dbias_slab, const int32_t *positions, const int32_t *offsets, float *dtable,
                          int32_t chunks, int32_t H, int32_t N, int32_t n_bins, int32_t accumulate, void *stream);

/* ---- row kernels (HBM-bound) ------------------------------------------------------------ */
/* nn.LayerNorm over the last dim (nets/ShfitScaleFormer.py:182-183, :902, :915, :926, :941;
 * vit_model.py:183-184, :498): x [rows, cols] fp32 -> y (y_dtype), saving mean / rstd [rows].
 * y_dtype == DM_BF16_PAIR (ABI 4, cols <= 1024): y is the hi / lo plane pair [2, rows, cols] of the result. */
int dm_layernorm_fwd(const float *x, const float *gamma, const float *beta, void *y, int32_t y_dtype,
                     float *mean, float *rstd, int32_t rows, int32_t cols, float eps, void *stream);
/* dx = (dres ? dres : 0) + LN'(dy); dx_lp (optional) receives the same values as bf16 (the operand
 * copy the previous layer's backward GEMMs consume); dgamma/dbeta (+)= column sums.  partial: fp32 scratch of
 * dm_layernorm_bwd_partial_floats(cols) floats. */
int dm_layernorm_bwd(const void *dy, int32_t dy_dtype, const float *x, const float *gamma,
                     const float *mean, const float *rstd, const float *dres, float *dx, void *dx_lp,
                     float *dgamma, float *dbeta, int32_t accumulate_params, float *partial,
                     int32_t rows, int32_t cols, void *stream);
int64_t dm_layernorm_bwd_partial_floats(int32_t cols);
/* The same backward WITHOUT the final reduction of the per-workgroup [dgamma | dbeta] partial rows: `*n_partial` rows of 2 * cols floats
 * are left in `partial` (keep it until they are reduced).  The reductions of a whole backward pass -- one per LayerNorm application,
 * nets/ShfitScaleFormer.py:170-183 runs two per block -- are then done by ONE dm_partial_reduce_batch launch instead of one small
 * launch each (out0 = dgamma, out1 = dbeta, width = 2 * cols, split = cols).  Results are bit-identical to dm_layernorm_bwd. */
int dm_layernorm_bwd_partials(const void *dy, int32_t dy_dtype, const float *x, const float *gamma,
                              const float *mean, const float *rstd, const float *dres, float *dx, void *dx_lp,
                              float *partial, int32_t rows, int32_t cols, int32_t *n_partial, void *stream);
/* The same with the hi / lo PLANE PAIR of dx on the side (dx_pair bf16 [2, rows, cols]; ABI 4): the gradient that leaves a LayerNorm
 * is the left operand of the next weight / data gradient products of the "bf16x3" mode, which then need no split pass.  cols <= 1024. */
int dm_layernorm_bwd_partials_pair(const void *dy, int32_t dy_dtype, const float *x, const float *gamma,
                                   const float *mean, const float *rstd, const float *dres, float *dx, void *dx_pair, float *partial,
                                   int32_t rows, int32_t cols, int32_t *n_partial, void *stream);
/* dm_layernorm_bwd_partials with the rows of the bf16 copy REGROUPED: rows = B * S * T, row (b, s, t) of dx is stored as row (s, b, t)
 * of dx_lp (bf16 [S, B, T, cols], required) -- the order in which the per-scale patch embeds read the token cube's gradient.  dx itself
 * and the partial rows are those of dm_layernorm_bwd_partials.  cols <= 1024. */
int dm_layernorm_bwd_partials_regroup(const void *dy, int32_t dy_dtype, const float *x, const float *gamma,
                                      const float *mean, const float *rstd, const float *dres, float *dx, void *dx_lp, float *partial,
                                      int32_t rows, int32_t cols, int32_t S, int32_t T, int32_t *n_partial, void *stream);
/* One job of dm_partial_reduce_batch: out0[j] (+)= sum_r partial[r][j] for j < split, out1[j - split] (+)= ... for split <= j < width;
 * rows are summed in a fixed order (deterministic).  Jobs of one batch must not share output elements. */
typedef struct DmReduceItem {
  const float *partial;
  float *out0, *out1;
  int32_t nrows, width, split, accumulate;
} DmReduceItem;
/* items: HOST array of n jobs (passed to the kernel by value, 32 per launch). */
int dm_partial_reduce_batch(const DmReduceItem *items, int32_t n, void *stream);

/* Per-scale 2x2 average pooling of the token grid (AvgPool2d(2,2) on [B,C,side,side] views,
 * nets/ShfitScaleFormer.py:892-901, :905-914): x [B, S*side*side, C] -> y [B, S*(side/2)^2, C], fp32. */
int dm_token_pool_fwd(const float *x, float *y, int32_t B, int32_t S, int32_t side, int32_t C, void *stream);
int dm_token_pool_bwd(const float *dy, float *dx, int32_t B, int32_t S, int32_t side, int32_t C, void *stream);
/* A stage transition, LayerNorm(pool(x)) (nets/ShfitScaleFormer.py:892-915), in ONE launch each way (additive entry points, ABI 7).
 * Forward: pooled [B, S*(side/2)^2, C] (kept for the backward pass), y = LayerNorm(pooled) fp32, mean / rstd per pooled row --
 * bit-identical to dm_token_pool_fwd followed by dm_layernorm_fwd(DM_F32).
 * Backward: dy fp32 [pooled rows, C] -> dx fp32 [B, S*side*side, C] and, when dx_lp is set, the same values rounded to bf16 --
 * bit-identical to dm_layernorm_bwd, dm_token_pool_bwd, dm_cast(DM_BF16).  dgamma / dbeta set: reduced here ((+)= with
 * accumulate_params); NULL: `*n_partial` partial rows are left in `partial` for dm_partial_reduce_batch, as dm_layernorm_bwd_partials
 * leaves them (same rows, same layout).  Only the widths dm_pool_layernorm_ok(C) accepts (768); others: DM_ERR_UNSUPPORTED. */
int dm_pool_layernorm_ok(int32_t C);
int dm_pool_layernorm_fwd(const float *x, const float *gamma, const float *beta, float *pooled, float *y, float *mean, float *rstd,
                          int32_t B, int32_t S, int32_t side, int32_t C, float eps, void *stream);
int dm_pool_layernorm_bwd(const float *dy, const float *pooled, const float *gamma, const float *mean, const float *rstd, float *dx,
                          void *dx_lp, float *dgamma, float *dbeta, int32_t accumulate_params, float *partial, int32_t *n_partial,
                          int32_t B, int32_t S, int32_t side, int32_t C, void *stream);
/* Mean over groups of `g` consecutive rows (AdaptiveAvgPool1d(1) per scale, :930-938):
 * x [rows*g, C] -> y [rows, C]; backward broadcasts dy/g. */
int dm_group_mean_fwd(const float *x, float *y, int32_t rows, int32_t g, int32_t C, void *stream);
int dm_group_mean_bwd(const float *dy, float *dx, int32_t rows, int32_t g, int32_t C, void *stream);

/* out[n] (+)= sum_m X[m,n]  (bias gradients).  partial: dm_colsum_partial_floats(N) floats. */
int dm_colsum(const void *X, int32_t dtype, int64_t ldx, float *out, int32_t M, int32_t N,
              int32_t accumulate, float *partial, void *stream);
int64_t dm_colsum_partial_floats(int32_t N);

/* fp32 -> T element-wise copy (weights / activations), n elements. */
int dm_cast(const float *src, void *dst, int32_t dst_dtype, int64_t n, void *stream);

/* Split-bf16 operand image for the "bf16x3" numerics mode: x = hi + lo with hi = bf16(x), lo = bf16(x - hi), so that an fp32
 * product A.B is recovered to ~2^-17 relative by ONE bf16 GEMM over a 3x longer contraction, [Ah | Ah | Al] . [Bh | Bl | Bh]
 * (the lo.lo term is dropped).  This replaces the reference's plain fp32 `nn.Linear` arithmetic (nets/ShfitScaleFormer.py:58-66,
 * :115-132) where bf16 alone misses the 1e-3 tolerance.  src fp32 [rows, cols] with leading dimension ld; dst bf16:
 *   stack = 0: [rows, 3*cols], piece j at column offset j*cols (the contraction runs along a row: NT's A and B, NN's A);
 *   stack = 1: [3*rows, cols], piece j at row offset j*rows    (the contraction runs down the rows: NN's B, TN's A and B).
 * pattern bit j set = piece j is the lo part: 0b100 for the left operand (hi, hi, lo), 0b010 for the right (hi, lo, hi).
 * cols % 4 == 0. */
int dm_split_bf16(const float *src, int64_t ld, int64_t rows, int64_t cols, void *dst, int32_t stack, int32_t pattern, void *stream);
/* The same with the column sums of src on the side (the bias gradient db = colsum(dy) that goes with dW = dy^T x,
 * nets/ShfitScaleFormer.py:58-66 under autograd: dy is read once for its split image and its sums): partial receives
 * *n_partial rows of `cols` floats (dm_split_colsum_partial_floats(rows, cols) floats at most), to be summed in row order --
 * e.g. by dm_partial_reduce_batch.  cols % 8 == 0, ld % 4 == 0, 16-byte aligned tensors (DM_ERR_UNSUPPORTED otherwise). */
int64_t dm_split_colsum_partial_floats(int64_t rows, int64_t cols);
/* The hi / lo PLANE PAIR of src: dst bf16 [2, rows, cols] (plane 0 = hi, plane 1 = lo, each with leading dimension cols), the operand
 * format of DmGemmArgs.k_fold.  partial / n_partial as for dm_split_bf16_colsum, or both NULL (no column sums).
 * cols % 8 == 0, ld % 4 == 0, 16-byte aligned tensors (DM_ERR_UNSUPPORTED otherwise). */
int dm_split_bf16_planes(const float *src, int64_t ld, int64_t rows, int64_t cols, void *dst, float *partial, int32_t *n_partial, void *stream);
int dm_split_bf16_colsum(const float *src, int64_t ld, int64_t rows, int64_t cols, void *dst, int32_t stack, int32_t pattern,
                         float *partial, int32_t *n_partial, void *stream);

/* Patch extraction for the k=stride Conv2d of PatchEmbed (nets/ShfitScaleFormer.py:25, :35):
 * x [B, C, side, side] fp32 -> cols [B*(side/p)^2, C*p*p] T, column order (c, dy, dx) = the
 * conv weight's [out, C, p, p] flattening, row order (b, py, px) = flatten(2).transpose(1,2). */
int dm_patchify(const float *x, void *cols, int32_t dtype, int32_t B, int32_t C, int32_t side, int32_t p, void *stream);

/* ---- loss / optimiser -------------------------------------------------------------------- */
/* Losses.py:34-38: d = sum((a-b)^2, 1); l = flag*d + (1-flag)*relu(margin-d); loss = mean(l).
 * Writes loss[0], and (if da/db != NULL) da = upstream*dloss/da, db likewise.  flag: fp32 [B]. */
int dm_contrastive_loss(const float *a, const float *b, const float *flag, float margin, float upstream,
                        float *loss, float *da, float *db, int32_t B, int32_t D, void *stream);

/* nn.CrossEntropyLoss, mean reduction (Losses.py:52-53 `MultiLoss.Loss_Class`, :83-84 `ClassLoss.Loss_Class`):
 * logits fp32 [B,K]; targets either class indices (int64 [B], target_prob NULL) or class probabilities
 * (fp32 [B,K], target_index NULL).  Writes loss[0] and, if dlogits != NULL, upstream * dloss/dlogits.
 * Out-of-range class indices are the caller's responsibility (torch raises; this reads out of bounds). */
int dm_cross_entropy(const float *logits, const int64_t *target_index, const float *target_prob, float upstream,
                     float *loss, float *dlogits, int32_t B, int32_t K, void *stream);

/* torch.optim.Adam single step over a flat fp32 buffer (Train_SMT.py:192-193, :300): in-place on
 * param/m/v; `step` is 1-based; if param_lp != NULL also writes the bf16 copy of the new weights.
 * grad_scale multiplies the gradient first (1/world_size after an RCCL sum all-reduce).
 * Hyper-parameters are doubles: torch derives 1-beta and the bias corrections in double precision
 * before rounding to fp32, and 1-0.999f differs from (float)(1-0.999) by 1.3e-5 relative. */
int dm_adam_step(float *param, const float *grad, float *m, float *v, void *param_lp, int64_t n,
                 int32_t step, double lr, double beta1, double beta2, double eps, double grad_scale, void *stream);

/* The same step for use inside a captured hipGraph: the two step-dependent scalars come from device memory,
 * hyper_dev = {lr / (1 - beta1^step), sqrt(1 - beta2^step)} (fp32[2]), which the host rewrites before each replay;
 * dm_adam_hyper computes that pair on the host exactly as dm_adam_step does. */
int dm_adam_hyper(int32_t step, double lr, double beta1, double beta2, float *hyper_host);
int dm_adam_step_dev(float *param, const float *grad, float *m, float *v, void *param_lp, int64_t n, const float *hyper_dev,
                     double beta1, double beta2, double eps, double grad_scale, void *stream);
/* ABI 6: the same, and the updated weights also as the hi / lo bf16 plane pair of the "bf16x3" products (param_hi[i] = bf16(p),
 * param_lo[i] = bf16(p - param_hi[i]): dm_split_bf16_planes' split): the next step's folded GEMMs read the pair the optimizer left instead of
 * splitting every weight matrix again (24 launches per step of the headline model). */
int dm_adam_step_dev_pair(float *param, const float *grad, float *m, float *v, void *param_hi, void *param_lo, int64_t n,
                          const float *hyper_dev, double beta1, double beta2, double eps, double grad_scale, void *stream);

/* ---- ExtractFeatures sweep ---------------------------------------------------------------- */
/* Per-superpixel mean pooling (ExtractFeatures.py:190-212): F [P,D] fp32, CSR ptr[S+1] / idx[*]
 * (int32) -> pooled [S,D]; rows are added in idx order then divided by the count (np.mean axis 0). */
int dm_segment_mean(const float *F, const int32_t *ptr, const int32_t *idx, float *pooled,
                    int32_t S, int32_t D, void *stream);
/* Per-edge distance (ExtractFeatures.py:139-147, :215-216): simi[e] = sqrt(max(0, |a|^2+|b|^2-2a.b))
 * for a = pooled[L], b = pooled[R]; edges int32 [E,2]; an edge with L == -1 or R == -1 yields NaN and
 * merge 0 (MyUtils2.py:184-186 skips them).  merge[e] = simi[e] < margin (uint8), may be NULL.
 * Summation order is fixed and documented in oracle/sweep_strict.c (bit-exact contract). */
int dm_edge_similarity(const float *pooled, const int32_t *edges, float *simi, uint8_t *merge,
                       int32_t E, int32_t D, float margin, void *stream);
/* Dense pairwise distance (ExtractFeatures.py:119-147 `Euclidean_distance`, called at :215; ExtractFeatures.py:228-237
 * `MC_Lyu_2020`; Train_SMT.py:115-131 `Euclidean_distance`): X [n,p], Y [m,p] row-major contiguous -> D [n,m] row-major,
 *   D[i,j] = sqrt(max(0, (x2[i] + y2[j]) - 2 xy[i,j]))   (NaN stays NaN; correctly rounded sqrt), one launch per call.
 * dtype DM_F32 (xy on the f32-input MFMA) or DM_F64 (fma(double) chains).  xy, x2 and y2 are the same k-ordered fma chain
 * from +0, so a row of X that equals a row of Y bit for bit gives exactly 0, and every entry depends on its two rows only
 * (same bits for any n, m, tile position or row subset).  n, m, p >= 1; n * m may exceed 2^31. */
int dm_pairwise_distance(const void *X, const void *Y, void *D, int32_t n, int32_t m, int32_t p, int32_t dtype, void *stream);

/* ---- patch pyramid gather --------------------------------------------------------------------
 * Replaces, for one scale, the per-point loader work of MyUtils1.py:116-223 / MyUtils2.py:286-437:
 * calculate_left_top_point_and_size (top-left = int(mid - L/2), truncation toward zero), cut_image (window
 * clipped to the raster, zero padded) and resize_data (per band resize to target x target on uint8, /255).
 * resize_rule: DM_RESIZE_OPENCV = cv::resize(..., INTER_AREA) on uint8 restated branch by branch (integer-ratio fast path incl. the
 * half-up 2x case, float area tables, 11-bit fixed-point bilinear with area coordinates when the window is smaller than the target);
 * DM_RESIZE_EXACT_AREA = the exact rational area average of rounds 1-2.  Both are specified in oracle/patches.py (no cv2 fixture
 * exists: the OpenCV rule is faithful to the published algorithm, unpinned against a build).
 *   tile [bands,H,W] uint8; xy int32 [P,2] = (XPixel, YLine); windows int32 [P] = window side L for this scale,
 *   every L <= max_window <= 384; out float32 [P, bands, target, target]. */
#define DM_RESIZE_OPENCV 0
#define DM_RESIZE_EXACT_AREA 1
int dm_patch_pyramid(const uint8_t *tile, int32_t bands, int32_t H, int32_t W, const int32_t *xy, const int32_t *windows,
                     int32_t max_window, int32_t P, int32_t target, int32_t resize_rule, float *out, void *stream);
/* The same gather emitting the patch-embed GEMM's operand rows directly ("patch pyramid gather fused into
 * patch-embed"): cols [P * grid * grid, bands * ps * ps] with ps = target / grid, row (p * grid + py) * grid + px, column
 * (c * ps + dy) * ps + dx -- the im2col order of Conv2d(k = ps, stride = ps) (nets/ShfitScaleFormer.py:28-37) -- in bf16 or
 * fp32.  Equal, bit for bit, to dm_patch_pyramid followed by dm_patchify. */
int dm_patch_pyramid_cols(const uint8_t *tile, int32_t bands, int32_t H, int32_t W, const int32_t *xy, const int32_t *windows,
                          int32_t max_window, int32_t P, int32_t target, int32_t grid, int32_t resize_rule, void *cols, int32_t dtype,
                          void *stream);

/* ---- training feed: one scale of a pair batch from resident tiles and a DEVICE sample table (ABI 5) -----------------------
 * Replaces, for the training loop, the host-side batch assembly of Train_SMT.py:212-262 (DataLoader items of MyUtils1.py:41-77:
 * get_scales :130-156, the crop / pad / resize chain :116-223, the designed-feature row :60-77) without any host round trip:
 * no window arithmetic on the host, no per-tile launches, nothing read back.  Sample p is cut from tile tile_id[p] (tiles uint8
 * [n_tiles, bands, H, W], tile_id may be NULL: one tile) around pixel xy[p] with the window side the reference derives from
 * inner[p] / obj[p]: (inner, obj, obj + (obj - inner), obj + 2 (obj - inner))[scale_index].  Same crop / pad / resize arithmetic
 * and results as dm_patch_pyramid / dm_patch_pyramid_cols, bit for bit.
 *   grid == 0: out float32 [P, bands, target, target];  grid > 0: out = patch-embed rows [P * grid * grid, bands * ps * ps],
 *   dtype DM_BF16 / DM_F32 (the layout of dm_patch_pyramid_cols).
 *   region_features [P, 15] + designed [P, 19] (both or neither): designed[p] = region_features[p] || window sides / (32, 64, 128, 1)
 *   (patches.CONFIG_SCALES, config.py:32) -- the `designed features` tensor of MyUtils1.py:74-77.
 *   max_window bounds the LDS staging (<= 384).  A sample whose tile id or window side is out of range produces zeros and sets
 *   error_flag[0] |= 1 (int32 on the device, may be NULL): the caller reads it when it reads the loss, not per step. */
int dm_pair_batch_gather(const uint8_t *tiles, int32_t n_tiles, int32_t bands, int32_t H, int32_t W, const int32_t *tile_id,
                         const int32_t *xy, const int32_t *inner, const int32_t *obj, int32_t scale_index, int32_t max_window,
                         int32_t P, int32_t target, int32_t grid, int32_t resize_rule, void *out, int32_t dtype,
                         const float *region_features, float *designed, int32_t *error_flag, void *stream);
/* Dihedral augmentation (additive in ABI 7): dm_pair_batch_gather with one orientation per sample, orient int32 [P] in 0..7 (not
 * NULL; both sides of a pair carry the same value).  With crop the zero-padded L x L window exactly as above,
 *   crop' = crop;  bit 1 set: crop' = crop'[::-1, :];  bit 0 set: crop' = crop'[:, ::-1];  bit 2 set: crop' = crop'.T
 * i.e. crop'[j][i] = crop[fy(a)][fx(b)] with (a, b) = (i, j) when bit 2 is set and (j, i) otherwise, fy mirroring (L - 1 - .) when
 * bit 1 is set and fx when bit 0 is set.  The resize (either rule) and / 255 then run on crop' unchanged: `out` is what
 * dm_pair_batch_gather writes for a tile whose window content is crop'.  The designed rows are not touched by the orientation (the 15
 * attributes are D4-invariant, the scale factors depend on window sides only); orient[p] == 0 is dm_pair_batch_gather's result.  A
 * sample whose orient is outside 0..7 is treated like a bad tile id: zeros, error_flag[0] |= 1, its designed row still written. */
int dm_pair_batch_gather_oriented(const uint8_t *tiles, int32_t n_tiles, int32_t bands, int32_t H, int32_t W, const int32_t *tile_id,
                                  const int32_t *xy, const int32_t *inner, const int32_t *obj, const int32_t *orient, int32_t scale_index,
                                  int32_t max_window, int32_t P, int32_t target, int32_t grid, int32_t resize_rule, void *out,
                                  int32_t dtype, const float *region_features, float *designed, int32_t *error_flag, void *stream);
/* Radiometric jitter (additive in ABI 7): dm_pair_batch_gather_oriented with one (gain, offset) per (sample, band) on top.
 *   radio   int32 [P, bands, 2], not NULL: gain is Q8 in 0 .. 1023 (256 = 1.0), offset is in 1/256 grey levels in -65535 .. 65535.
 *           Both sides of a pair carry the same values (two views of one scene under one illumination).
 *   orient  as above, or NULL: every orientation 0.
 * Pixels.  Every pixel v of the zero-padded L x L crop that lies inside the raster becomes
 *   v' = min(255, max(0, (gain v + offset + 128) >> 8))        (int32; the shift is arithmetic: floor for negative sums)
 * and padding pixels stay 0 whatever the offset.  |gain v + offset + 128| < 2^19.  The rule is per pixel, so it commutes with the
 * dihedral index map; orientation, either resize rule and / 255 then run on the transformed crop unchanged.
 * Designed row (written when region_features / designed are given).  With the attributes in oracle/rag.py's order -- std at 5..7,
 * means at 8..10, bright at 13 -- nb = min(bands, 3), and for c < nb, in fp32, round to nearest, no contraction:
 *   gf = (float)gain_c / 256,  bf = (float)offset_c / 256                       (both exact)
 *   mean_c' = min(255, max(0, gf mean_c + bf)),   std_c' = gf std_c
 *   bright' = bright + (((mean_0' - mean_0) + (mean_1' - mean_1)) + (mean_2' - mean_2)) / (float)nb     (left to right over c < nb)
 * Attributes of bands >= nb, the other ten attributes and the four scale factors are not touched.  The identity table (256, 0)
 * leaves the row bit for bit as dm_pair_batch_gather_oriented writes it.  First order: pixels that clamp are not accounted for in
 * std'; the attributes are taken to be on the 0..255 scale of the tile bytes (rag.label_stats).
 * A sample with a gain or an offset of any band outside its range is treated like a bad orientation: zeros in every band,
 * error_flag[0] |= 1, its designed row written from the untransformed attributes; no other sample is affected. */
int dm_pair_batch_gather_augmented(const uint8_t *tiles, int32_t n_tiles, int32_t bands, int32_t H, int32_t W, const int32_t *tile_id,
                                   const int32_t *xy, const int32_t *inner, const int32_t *obj, const int32_t *orient,
                                   const int32_t *radio, int32_t scale_index, int32_t max_window, int32_t P, int32_t target, int32_t grid,
                                   int32_t resize_rule, void *out, int32_t dtype, const float *region_features, float *designed,
                                   int32_t *error_flag, void *stream);

/* ---- per-epoch pair draw: the epoch's whole sample table in one launch (additive in ABI 6) ---------------------------------
 * Replaces the dataset rebuild of every epoch (MyUtils1.py:275-293: for each pair of the positive / negative lists, one sample
 * point drawn uniformly from each polygon's `PointID` list) and the shuffled loader over it (Train_SMT.py:218-220:
 * DataLoader(shuffle=True), drop_last=False) with a counter-based draw keyed by (seed, epoch) -- DESIGN.md 3.9 states the
 * Philox4x32-10 / Feistel contract.  Nothing is read back.
 *   pairs int32 [N, 2] global polygon ids, pair_flag int32 [N] (1 = merge); polygon -> points CSR poly_off int32 [n_poly + 1],
 *   poly_pts int32 [n_poly_pts]; point table pt_tile int32 [n_pts], pt_xy int32 [n_pts, 2] (pixels), pt_inner / pt_obj int32
 *   [n_pts], pt_region float32 [n_pts, 15].
 *   Output in per-step blocked layout: position j belongs to step s = j / batch with b_s = min(batch, N - s batch) pairs; its
 *   left sample goes to row 2 s batch + (j - s batch), its right sample to that row + b_s (rows [2 s batch, 2 s batch + 2 b_s)
 *   are step s's feed.PairTable).  tile_id int32 [2N], xy int32 [2N, 2], inner / obj int32 [2N], region float32 [2N, 15],
 *   flag float32 [N] in position order, point_id int32 [2N] (may be NULL).  A polygon id, point list or point id out of range
 *   reads nothing out of range: that sample gets point_id -1, tile id -1 and zeros. */
typedef struct {
  const int32_t *pairs, *pair_flag, *poly_off, *poly_pts;
  const int32_t *pt_tile, *pt_xy, *pt_inner, *pt_obj;
  const float *pt_region;
  int32_t *tile_id, *xy, *inner, *obj;
  float *region, *flag;
  int32_t *point_id;
  uint64_t seed;
  int32_t n_pairs, n_poly, n_poly_pts, n_pts, epoch, batch;
} DmPairDraw;
int dm_pair_epoch_draw(const DmPairDraw *args, void *stream);
/* The epoch's orientation column for dm_pair_batch_gather_oriented (additive in ABI 7), in the same blocked layout: the pair at
 * shuffled position j, src = perm(j), gets philox4x32_10((src, epoch, 3, 0), key)[0] & mask -- key and perm as in
 * dm_pair_epoch_draw, counter word 3 a stream neither the draw (1) nor the shuffle (2) uses -- written to both of its rows,
 * row_l and row_l + b_s.  mask: 7 (the dihedral group D4) or 3 (flips only, no transposition).  Keyed by (seed, epoch, pair): a
 * resumed run sees the same orientations.  orient int32 [2 n_pairs].  Refused before any launch: another mask, n_pairs outside
 * 1 .. 2^30, batch < 1, epoch < 0, a null pointer. */
int dm_pair_epoch_orient(uint64_t seed, int32_t epoch, int32_t n_pairs, int32_t batch, int32_t mask, int32_t *orient, void *stream);
/* The epoch's radiometric table for dm_pair_batch_gather_augmented (additive in ABI 7), radio int32 [2 n_pairs, bands, 2] in the same
 * blocked layout, drawn from counter word 4 (neither the draw's, the shuffle's nor the orientation's).  With src = perm(j) and
 *   sym(r, s) = (int32)umulhi(r, 2 s + 1) - s                                   (uniform on -s .. s; 0 when s = 0)
 *   A = philox4x32_10((src, epoch, 4, 0), key):   g0 = 256 + sym(A[0], gain_span),   b0 = sym(A[1], offset_span)
 *   band c:  B = philox4x32_10((src, epoch, 4, 1 + c / 4), key)[c % 4],   gain_c = g0 + sym(B, band_span),
 *            offset_c = b0 - 128 (gain_c - 256)                                  (the contrast pivots about mid-grey)
 * (gain_c, offset_c) goes to both rows of the pair, row_l and row_l + b_s.  Within the span limits below every gain lies in
 * 64 .. 448 and every |offset| <= 40896: in range by construction.  Refused before any launch: a span below 0 or over its limit,
 * bands outside 1 .. 16, n_pairs outside 1 .. 2^30, batch < 1, epoch < 0, a null pointer. */
#define DM_RADIO_MAX_GAIN_SPAN 128
#define DM_RADIO_MAX_BAND_SPAN 64
#define DM_RADIO_MAX_OFFSET_SPAN 16320
int dm_pair_epoch_radiometric(uint64_t seed, int32_t epoch, int32_t n_pairs, int32_t batch, int32_t bands, int32_t gain_span,
                              int32_t band_span, int32_t offset_span, int32_t *radio, void *stream);
/* Weighted pair sampling with replacement (additive in ABI 7; DESIGN.md 3.9, tests/sampling_ref.py restates it in numpy).
 * w int64 [N] weights, all >= 0 and not all 0; cum = the inclusive prefix sums of w (int64 [N]); T = cum[N - 1], 1 <= T < 2^62 (the
 * caller validates w and T; deepmerge_amd.dataset does, with one readback per epoch).  M draws, 1 <= M <= 2^30; N <= 2^30.
 * Select -- counter word 5, which the draw (1), shuffle (2), orientation (3) and jitter (4) do not use.  For position j in [0, M):
 *   r = philox4x32_10((j, epoch, 5, 0), key),   R = (uint64)r[0] << 32 | r[1],   u = umul64hi(R, T)        (0 <= u < T)
 *   src[j] = #{i : cum[i] <= u} = the smallest i with cum[i] > u
 * so a pair of weight 0 is never selected wherever it sits.  src int32 [M].  One thread per position, a binary search whose index
 * stays in [0, N) for ANY cum: a table that breaks the contract reads nothing out of range and yields values in [0, N] (N: see
 * below).  Refused before any launch: a null pointer, n_pairs or n_draws outside 1 .. 2^30, epoch < 0. */
int dm_pair_epoch_select(const int64_t *cum, int32_t n_pairs, int32_t n_draws, uint64_t seed, int32_t epoch, int32_t *src, void *stream);
/* The sampled epoch: position j of n_draws takes pair src[j] (src int32 [n_draws], e.g. dm_pair_epoch_select's).  A pair can be drawn
 * twice in one epoch, and must not show the same sample points, orientation and exposure twice, so the three streams are keyed by
 * the POSITION j, on counter words of their own (the unsampled word + 16):
 *   point draw   r = philox4x32_10((j, epoch, 17, 0), key), r[0] / r[1] used as dm_pair_epoch_draw uses them
 *   orientation  philox4x32_10((j, epoch, 19, 0), key)[0] & mask
 *   radiometric  A = philox4x32_10((j, epoch, 20, 0), key),  B = philox4x32_10((j, epoch, 20, 1 + c / 4), key), sym and limits as above
 * Everything is a function of (seed, epoch, j, w): independent of the batch size, the same after a resume given the same weights.
 * Layout: the blocked layout above with n_draws in place of N (b_s = min(batch, n_draws - s batch)); flag[j] = pair_flag[src[j]].
 * args->n_pairs stays the list length N; the outputs hold 2 n_draws rows and n_draws flags.  An src entry outside [0, N) reads
 * nothing out of range: both samples of the position get point_id -1, tile id -1 and zeros, and flag[j] = 0.  The same kernels as
 * the unsampled entry points, instantiated on the key rule; refusals as theirs, plus a null src and n_draws outside 1 .. 2^30. */
int dm_pair_epoch_draw_src(const DmPairDraw *args, const int32_t *src, int32_t n_draws, void *stream);
int dm_pair_epoch_orient_src(uint64_t seed, int32_t epoch, int32_t n_draws, int32_t batch, int32_t mask, int32_t *orient, void *stream);
int dm_pair_epoch_radiometric_src(uint64_t seed, int32_t epoch, int32_t n_draws, int32_t batch, int32_t bands, int32_t gain_span,
                                  int32_t band_span, int32_t offset_span, int32_t *radio, void *stream);

/* ---- held-out pair evaluation (additive in ABI 6; deepmerge_amd/evaluate.py) ---------------------------
 * Per-pair contrastive terms -- the per-pair form of the reference's contrastive loss (Losses.py:34-38, before its mean):
 *   d2[r] = sum_c (a[r,c] - b[r,c])^2,   term[r] = f*d2 + (1-f)*max(margin - d2, 0),   f = flag[r]
 * a, b [B, D] fp32 row-major, flag / d2 / term [B] fp32.  The order is pinned (no FMA contraction): lane l of the pair's wave
 * sums its columns l, l+64, ... in order, the partials are combined by the xor butterfly 32, 16, ..., 1, then the term is
 * evaluated left to right (a NaN d2 gives a NaN term).  B, D >= 1 (DM_ERR_BAD_SHAPE). */
int dm_contrastive_terms(const float *a, const float *b, const float *flag, float margin, float *d2, float *term, int32_t B, int32_t D,
                         void *stream);
/* One pass over the N pairs of an evaluation -- what the reference meant to log per epoch as val_loss / f_score
 * (callbacks.py:41-57 `append_loss`, called at Train_SMT.py:350 with the training loss and the elapsed time in their place):
 *   merged[0][j] = #{r : flag[r] == 1 and simi[r] < thresholds[j]},  merged[1][j] the same for flag[r] != 1   (int64 [2, T])
 *   n_pos = #{r : flag[r] == 1},   loss_sum = sum_r term[r] in fp64
 * The merge rule is the sweep's (`simi < margin`): simi == t does not merge and a NaN simi never merges.  thresholds fp32 [T] on
 * the device, finite and strictly ascending (the caller checks), 1 <= T <= 1024 (DM_ERR_UNSUPPORTED); 1 <= N <= 2^31 - 1
 * (DM_ERR_BAD_SHAPE).  Counts are exact; loss_sum is summed over a partition that depends on N only, in a fixed order (bit-identical
 * from run to run).  workspace: dm_pair_eval_workspace_bytes(N, T) bytes, 8-byte aligned.  No host synchronisation. */
int64_t dm_pair_eval_workspace_bytes(int64_t N, int32_t T);
int dm_pair_eval_summary(const float *term, const float *simi, const float *flag, int64_t N, const float *thresholds, int32_t T,
                         void *workspace, double *loss_sum, int64_t *merged, int64_t *n_pos, void *stream);

/* ---- region-adjacency graph + superpixel statistics from a label raster ---------------------------
 * Replaces, on the device, the inputs the reference reads from files written by external GIS software: the RAG edge
 * list (`LEFT_FID` / `RIGHT_FID` of lines.shp, MyUtils2.py:155-193, consumed at ExtractFeatures.py:188-219) and the 15
 * designed attributes (MyUtils1.py:79-114).  The definitions are this build's (oracle/rag.py); all results are exact
 * integers or fixed double-precision formulas of exact integers.
 *   labels int32 [H,W] (superpixel id, ids outside [0,S) are ignored); tile uint8 [bands,H,W].
 * dm_label_stats: count[S], sum / sumsq [S, min(bands,3)] (int64), bbox int32 [S,4] = xmin,ymin,xmax,ymax
 *   (INT_MAX,INT_MAX,-1,-1 for an id that never occurs), peri int64 [S,2] = pixel edges shared with another label /
 *   lying on the raster border.  All outputs are (re)initialised by the call.  The id -2 is RESERVED: it is the pass's own
 *   marker for "outside the raster", so a pixel that carries it is ignored like every id outside [0,S), and the pixel edges
 *   its four neighbours share with it count as raster border (column 1), not as shared with another label.  The raster is
 *   not searched for it.
 * dm_label_features: float32 [S,15] = area, peri, len, width, smooth, std0..2, mean0..2, shapeness, compact, bright,
 *   border (the attribute order of MyUtils1.py:79-114).
 * dm_rag_edges: unique unordered 4-neighbour label pairs a < b as keys a*S+b with the number of shared pixel edges.
 *   table_keys / table_counts: scratch of 2^capacity_log2 entries (int64 / int32); edge_keys / edge_counts: up to
 *   max_edges results in ARBITRARY order (sort by key for a canonical list); n_edges[0] = number found (may exceed
 *   max_edges: then the output is truncated); overflow[0] = 1 if the table was too small. */
int dm_label_stats(const int32_t *labels, const uint8_t *tile, int32_t bands, int32_t H, int32_t W, int32_t S,
                   int64_t *count, int64_t *sum, int64_t *sumsq, int32_t *bbox, int64_t *peri, void *stream);
int dm_label_features(const int64_t *count, const int64_t *sum, const int64_t *sumsq, const int32_t *bbox, const int64_t *peri,
                      int32_t S, int32_t bands, float *features, void *stream);
int dm_rag_edges(const int32_t *labels, int32_t H, int32_t W, int32_t S, int64_t *table_keys, int32_t *table_counts,
                 int32_t capacity_log2, int64_t *edge_keys, int32_t *edge_counts, int32_t max_edges, int32_t *n_edges,
                 int32_t *overflow, void *stream);

/* ---- seam stitch: the graph and the perimeters between the tiles of a scene (additive in ABI 7; csrc/dm_scene.hip, DESIGN.md
 * 3.5.9, rag.seam_stitch / deepmerge_amd/scene.py) ------------------------------------------------------------------------------
 * A scene larger than one raster is segmented tile by tile; superpixels never cross a seam and carry scene-wide ids 0..S-1.
 * dm_label_stats and dm_rag_edges run per tile, so they miss what lies between tiles.  This call adds it, so that the
 * concatenated per-tile results equal what the two calls give on the assembled scene raster, bit for bit.
 * The rule.  a, b int32 [n]: a[i] and b[i] are the scene-wide ids of the two pixels that face each other across seam position
 * i; all seams of the scene are concatenated, in any order.  1 <= n, 1 <= S <= 2^24.
 *   edges: every position with both ids in [0,S) and a[i] != b[i] adds 1 to key min*S + max: dm_rag_edges' key and count for a
 *     4-neighbour pair, through the same table.  With per-tile superpixels the pairs are disjoint from every tile's own (a
 *     tile's pairs lie inside it); with a label raster whose regions cross seams (scene.label_graph) a pair can
 *     occur in several tiles and on seams, and the caller adds the weights of equal keys.
 *   perimeter: peri int64 [S,2] holds dm_label_stats' peri of every tile, concatenated.  The tile counted the pixel edge of
 *     a[i] that faces b[i] in column 1 (raster border); dm_label_stats on the scene would see the neighbour b[i].  So, for the
 *     side l = a[i] facing f = b[i], and likewise for l = b[i] facing f = a[i], when l is in [0,S):
 *       f == -2 (dm_label_stats' marker for "outside the raster"): nothing moves;
 *       f == l: column 1 loses the edge (inside a raster, equal neighbours share no perimeter): a region that crosses the seam;
 *       any other f, ids outside [0,S) such as -1 included: the edge moves from column 1 to column 0 ("another label").
 *     A side whose own id is outside [0,S) has no row in peri and moves nothing.
 * Integer adds only: nothing depends on arrival order.  table_* / edge_* / n_edges / overflow: as dm_rag_edges takes them
 * (8 <= capacity_log2 <= 30, results in ARBITRARY order, n_edges may exceed max_edges: then the output is truncated); they are
 * (re)initialised by the call, peri is updated in place.  Validates before any launch, never synchronises, never allocates. */
int dm_seam_stitch(const int32_t *a, const int32_t *b, int64_t n, int64_t S, int64_t *peri, int64_t *table_keys,
                   int32_t *table_counts, int32_t capacity_log2, int64_t *edge_keys, int32_t *edge_counts, int32_t max_edges,
                   int32_t *n_edges, int32_t *overflow, void *stream);

/* One round of the merge step that follows the sweep (optional; the reference leaves merging to external
 * GIS tooling): union-find over the edges with merge[e] != 0.  parent int32 [S] (init != 0: reset to the identity first);
 * after the call parent[s] is a root candidate and changed[0] tells whether any root was hooked -- repeat with init = 0
 * until changed[0] == 0; then parent[s] = the smallest superpixel id of s's component (order-independent). */
int dm_merge_round(const int32_t *edges, const uint8_t *merge, int32_t E, int32_t S, int32_t *parent, int32_t *changed,
                   int32_t init, void *stream);

/* ---- mutual-best-neighbour region merging (additive in ABI 6; csrc/dm_merge.hip, DESIGN.md 3.5, rag.merge_regions) -------
 * The rule.  State of a round: C regions with dense ids 0..C-1, point lists ptr int32 [C+1] / idx int32 [P], edges int32 [E,2]
 * with a < b, sorted by (a, b), unique, weights int32 [E] (shared boundary length), statistics as dm_label_stats writes them,
 * rep int32 [C] = the smallest ORIGINAL superpixel id inside each region.
 *   1. score: pooled = dm_segment_mean, simi = dm_edge_similarity (unchanged).
 *   2. best neighbour: an edge is a candidate iff simi < margin (float compare; NaN is none).  best[r] = the smallest key
 *      (bits(simi) << 32) | other_id over the candidate edges at r, as an unsigned 64-bit integer (simi >= +0, so the bit pattern
 *      orders like the value; ties go to the smaller neighbour id); all-ones = no candidate.
 *   3. match: edge (a, b) is picked iff best[a] names b and best[b] names a.  Picked edges form a matching (two picked edges
 *      sharing r would give best[r] two values); b is absorbed into a.
 *   4. fold: new dense ids in order of the surviving region's old id; new point list = points of a, then points of b, each in
 *      their old order; edges relabelled, self edges dropped, duplicates folded with their weights ADDED, sorted by (a, b);
 *      count / sum / sumsq added, bbox min / max, peri[:,1] added, peri[:,0]' = peri_a + peri_b - 2 weight(a, b); rep' = rep[a].
 *   5. history: one row per picked edge, in edge order within the round: (round, rep[a], rep[b]) int32 and simi float32.
 * All results are integers or floats copied bit for bit; every reduction is an integer min / add (order-independent).
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates.
 *
 * The elimination rule (minimum region area, additive in ABI 7; spec tests/merge_small_ref.py).  With min_area = A >= 1 the rounds
 * above run until one picks nothing; only then (not after max_rounds or min_regions ended them) elimination rounds follow.  Region
 * r is small iff count[r] < A (int64; count 0 is small, count == A is not).  A round replaces step 2 by:
 *   2a. propose: an edge is usable iff simi == simi (NaN never is; there is no margin).  Every small region s takes best[s] = the
 *       smallest key (bits(simi) << 32) | other_id over its usable edges, whatever the size of the other end; a non-small region
 *       gets all-ones.
 *   2b. accept: a non-small region t takes best[t] = the smallest key (bits(simi) << 32) | s over the small regions s whose best[s]
 *       names t, all-ones if there is none.
 * Steps 1 and 3 to 5 are unchanged: an edge is picked iff its two regions name each other, so two small regions merge only when
 * they propose to each other, and a small region whose choice proposed or accepted elsewhere waits a round.  best[r] is still one
 * value per region, so the picks are a matching.  The rounds stop when one picks nothing (then no small region has a usable edge),
 * at max_rounds (which counts both kinds of round), or before a round that would leave fewer than min_regions regions.  They do
 * not go back to the margin rule.
 *
 * dm_merge_best: best uint64 [C] (cleared by the call), one pass over the E >= 1 edges.  1 <= C <= 2^24.
 * dm_merge_best_small: step 2a; count int64 [C], min_area >= 1; best is cleared by the call.  dm_merge_accept: step 2b, in place on
 *   the best that dm_merge_best_small left, in a launch after it on the same stream (it reads entries of small regions and writes
 *   entries of non-small ones only).
 * dm_merge_match: picked uint8 [E]; root int32 [C] (root[b] = a for a picked edge, else the identity); pick int32 [C] = index of
 *   the picked edge at its surviving region a, else -1; n_picked[0] = number of picked edges.  All (re)initialised by the call.
 * dm_merge_fold_regions: step 4 for regions and step 5 (see DmMergeFold).  dm_merge_edge_keys + dm_merge_fold_edges: step 4 for
 *   edges, around a sort of the keys that the caller provides (any stable or unstable ascending sort of int64):
 *   keys[e] = (min(na, nb) << 32) | max(na, nb) for na = new_id[root[a]] != nb, INT64_MAX for a self edge;
 *   dm_merge_fold_edges(sorted keys, order = source index of every sorted key, weights or NULL) -> new_edges [n,2], new_weights [n],
 *   n_edges[0] = n.  One looping workgroup does the scan of either fold (DESIGN.md 3.5 states what that costs).
 * dm_relabel_raster: out[i] = map[labels[i]] for n int32 pixels, ids outside [0, S) copied through; 16-byte accesses when both
 *   rasters are 16-byte aligned, a scalar kernel for the tail or for unaligned rasters.  out may not alias labels partially. */
typedef struct {
  /* the round's state (read only) */
  const int32_t *ptr, *idx, *edges, *root, *pick, *rep, *region_of;   /* region_of int32 [S0]: current region of every original id */
  const float *simi;                                                  /* [E], this round's scores */
  const int32_t *weights;                                             /* [E]; needed only with statistics */
  const int64_t *count, *sum, *sumsq;                                 /* statistics: all five or count == NULL (none) */
  const int32_t *bbox;
  const int64_t *peri;
  /* results; new_id [C] is written for surviving regions only (an absorbed region's id is new_id[root[r]]), hist_rank [C] scratch */
  int32_t *new_id, *hist_rank, *new_ptr, *new_idx, *new_rep, *new_region_of, *n_regions;
  int64_t *new_count, *new_sum, *new_sumsq;
  int32_t *new_bbox;
  int64_t *new_peri;
  int32_t *history;                                                   /* int32 [hist_cap, 3]; rows hist_base .. are this round's */
  float *history_simi;                                                /* float32 [hist_cap] */
  int32_t C, P, E, S0, bands, round, hist_base, hist_cap;
} DmMergeFold;
int dm_merge_best(const int32_t *edges, const float *simi, int32_t E, int32_t C, float margin, uint64_t *best, void *stream);
int dm_merge_best_small(const int32_t *edges, const float *simi, int32_t E, int32_t C, const int64_t *count, int64_t min_area,
                        uint64_t *best, void *stream);
int dm_merge_accept(const int32_t *edges, const float *simi, int32_t E, int32_t C, const int64_t *count, int64_t min_area,
                    uint64_t *best, void *stream);
int dm_merge_match(const int32_t *edges, const uint64_t *best, int32_t E, int32_t C, uint8_t *picked, int32_t *root, int32_t *pick,
                   int32_t *n_picked, void *stream);
int dm_merge_fold_regions(const DmMergeFold *args, void *stream);
int dm_merge_edge_keys(const int32_t *edges, const int32_t *root, const int32_t *new_id, int32_t E, int32_t C, int64_t *keys,
                       void *stream);
int dm_merge_fold_edges(const int64_t *sorted_keys, const int64_t *order, const int32_t *weights, int32_t E, int32_t *new_edges,
                        int32_t *new_weights, int32_t *n_edges, void *stream);
int dm_relabel_raster(const int32_t *labels, const int32_t *map, int32_t *out, int64_t n, int32_t S, void *stream);

/* ---- multiresolution region merging (additive in ABI 7; csrc/dm_mrs.hip, DESIGN.md 3.5.8, rag.mrs) --------------------------
 * The classical baseline of a learned merge: the Baatz-Schaepe colour / shape heterogeneity criterion, driven by the mutual-best
 * merge above.  The rule.  State of a round: the state above without point lists (ptr all zeros, P = 0): C regions, edges,
 * weights = shared boundary length, and the five statistics of dm_label_stats for nb = min(bands, 3) bands.  Exact integers:
 *   region r:        n_r = count[r];  l_r = peri[r,0] + peri[r,1];  b_r = 2 ((x1 - x0 + 1) + (y1 - y0 + 1)) from bbox[r];
 *                    V_r,c = n_r sumsq[r,c] - sum[r,c]^2  (= (n sigma)^2, never negative)
 *   union m of edge (a, b, w):  n_m = n_a + n_b;  sum, sumsq added;  l_m = l_a + l_b - 2 w;  b_m from the union of the boxes.
 * V needs up to 78 bits (count up to 2^31): it is formed in 128-bit integers and converted to double with ONE rounding to
 * nearest-even (hi = V >> 32 < 2^46 and lo = V & 0xffffffff convert exactly, double(hi) * 2^32 is exact, the add rounds).
 * n, l, b are converted to double one by one.  Then, in IEEE double operations, no FMA contraction, in exactly this association:
 *   hc  = 0.0;  for c in 0..nb-1:  hc = hc + bw[c] * ((sqrt(V_m,c) - sqrt(V_a,c)) - sqrt(V_b,c))
 *   hcm = (l_m * sqrt(n_m) - l_a * sqrt(n_a)) - l_b * sqrt(n_b)                 compactness: n * l / sqrt(n)
 *   hsm = ((n_m * l_m) / b_m - (n_a * l_a) / b_a) - (n_b * l_b) / b_b           smoothness:  n * l / b
 *   hs  = compactness * hcm + (1.0 - compactness) * hsm
 *   f   = (1.0 - shape) * hc + shape * hs
 *   cost = float32(f > 0.0 ? f : 0.0)
 * The clamp to +0.0 is part of the rule: a merge that shortens the outline makes the shape term negative, and dm_merge_best
 * orders candidates by the bit pattern of a non-negative float.  All non-positive costs are equally best; ties go to the smaller
 * neighbour id.  An edge is a candidate iff cost < float32(scale * scale) (float compare); steps 2 to 5 above follow unchanged,
 * with simi = cost in the history.  shape in [0, 1), compactness in [0, 1], band weights finite and >= 0, none normalised.
 *
 * dm_region_merge_cost: cost float32 [E] of the E >= 1 edges, one thread per edge; 1 <= C <= 2^24, bands in 1..3 (= nb; bw of a
 *   band >= nb is checked and not used).  An edge with an endpoint outside [0, C) or with an empty region (count <= 0: it has no
 *   cost) gets NaN, which is never a candidate.
 * dm_pixel_regions: the start state in which pixel (y, x) of tile uint8 [bands,H,W] is region y W + x, in closed form: count 1,
 *   sum = p, sumsq = p^2 for the first nb bands, bbox = the pixel, peri = (4-neighbours inside the raster, 4 minus that).  Pixel a
 *   owns the edges (a, a + 1) if x + 1 < W, then (a, a + W) if y + 1 < H; its first edge is row y (2W - 1) + 2x of the list for
 *   y + 1 < H and row y (2W - 1) + x on the last row, so edges int32 [E,2] comes out sorted and unique, E = H (W - 1) + (H - 1) W,
 *   weights int32 [E] all 1.  1 <= H W <= 2^24; edges / weights may be NULL only for a 1 x 1 raster.  The result equals
 *   dm_label_stats and dm_rag_edges (sorted) of the raster labels[y,x] = y W + x bit for bit.
 * Both validate before any launch, launch on `stream`, never synchronise and never allocate. */
int dm_region_merge_cost(const int64_t *count, const int64_t *sum, const int64_t *sumsq, const int32_t *bbox, const int64_t *peri,
                         const int32_t *edges, const int32_t *weights, int32_t E, int32_t C, int32_t bands, double bw0, double bw1,
                         double bw2, double shape, double compactness, float *cost, void *stream);
int dm_pixel_regions(const uint8_t *tile, int32_t bands, int32_t H, int32_t W, int64_t *count, int64_t *sum, int64_t *sumsq,
                     int32_t *bbox, int64_t *peri, int32_t *edges, int32_t *weights, void *stream);

/* ---- sample points and window sides from a label raster (additive in ABI 6; csrc/dm_points.hip, DESIGN.md 3.5.2,
 * rag.clearance / rag.sample_points) ------------------------------------------------------------------------------------------
 * Replaces, on the device, the point shapefile the reference reads (pixel position and the `inner` / `object` window fields,
 * MyUtils1.py:64-66, MyUtils2.py:234-236, and the polygons' `PointID` lists).  The reference never defines these; the rule is
 * this build's (restated in numpy in tests/points_ref.py).  All arithmetic is on integers; results are bit-exact.
 * The rule.  labels int32 [H,W], H*W < 2^31, S superpixel ids 0..S-1, 1 <= k <= 16, 1 <= max_window <= 384.  Ids outside
 * [0,S) are never sampled but are "another label" to their neighbours (raw ids are compared).
 *   clearance: c(p) = Chebyshev distance from pixel p to the nearest pixel that carries a different id or lies outside the
 *     raster, capped at cap = (max_window + 1) / 2.  c >= 1; the largest odd square centred on p inside p's superpixel has
 *     side 2c - 1 (up to the cap).
 *   points: superpixel s gets min(k, area(s)) points in rounds j = 0..k-1.  Round j takes the pixel of s with the largest
 *     score_j(p) = min(c(p), Chebyshev distance from p to every point already chosen for s); ties go to the smallest linear
 *     index y*W + x; a round yields a point only if its best score is >= 1 (chosen pixels score 0).  As a 64-bit key
 *     (score << 32) | (0xFFFFFFFF - linear) a round is one unsigned integer max per superpixel.
 *   windows: inner = 2 c(p) - 1; side = max(bbox width, bbox height) of s; obj = min(side, (max_window + 2 inner) / 3).
 *     Hence inner <= obj and 3 obj - 2 inner (the largest of the four window sides get_scales derives) <= max_window.
 *   order: points sorted by (superpixel, round); ptr int32 [S+1] = exclusive scan of the per-superpixel counts.
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates.
 *
 * dm_label_clearance: the clearance rule.  clearance uint16 [H,W]; scratch: bits uint64 [H * ceil(W/64)] (one bit per pixel:
 *   has an 8-neighbour of another id or is on the raster edge), row_dist uint8 [H,W] (distance to the nearest such pixel of
 *   the row, capped at cap - 1).
 * dm_point_select_round: round `round` (0..k-1, to be called in that order) of the points rule over the whole raster.
 *   State: best uint64 [S], points int32 [S,k,2] = (x, y), point_clearance int32 [S,k] = c at the point, counts int32 [S],
 *   bbox int32 [S,4] = xmin,ymin,xmax,ymax (INT_MAX,INT_MAX,-1,-1 for an id that never occurs, as dm_label_stats writes it).
 *   Round 0 (re)initialises best, counts and bbox and computes bbox; every round appends at most one point per superpixel.
 * dm_point_emit: the windows and order rules.  ptr int32 [S+1]; xy int32 [capacity,2], label / inner / obj / round int32
 *   [capacity]: rows 0 .. ptr[S]-1 are written (capacity >= ptr[S]; S*k always suffices), round = the point's round j. */
int dm_label_clearance(const int32_t *labels, int32_t H, int32_t W, int32_t max_window, uint64_t *bits, uint8_t *row_dist,
                       uint16_t *clearance, void *stream);
int dm_point_select_round(const int32_t *labels, const uint16_t *clearance, int32_t H, int32_t W, int32_t S, int32_t k, int32_t round,
                          uint64_t *best, int32_t *points, int32_t *point_clearance, int32_t *counts, int32_t *bbox, void *stream);
int dm_point_emit(const int32_t *counts, const int32_t *points, const int32_t *point_clearance, const int32_t *bbox, int32_t S, int32_t k,
                  int32_t max_window, int32_t capacity, int32_t *ptr, int32_t *xy, int32_t *label, int32_t *inner, int32_t *obj,
                  int32_t *round, void *stream);

/* ---- sample points of a scene's label raster across tile seams (additive in ABI 7; csrc/dm_scene_points.hip, DESIGN.md 3.5.14,
 * scene.sample_points) ---------------------------------------------------------------------------------------------------------
 * A scene's label raster lives on the host and its regions know nothing of the tile grid: a region's pixels lie in several
 * tiles.  The rule is the points rule above, word for word, with "linear index" read as the SCENE's y*W + x and every distance
 * taken in scene coordinates, so the result equals dm_point_select_round / dm_point_emit on the whole raster bit for bit,
 * whatever the tiles.  Scene: H, W < 2^31 and H*W <= 2^48 (DM_SCENE_POINTS_MAX_PIXELS).
 *   state, scene-wide, on the device for all rounds: best uint64 [S], points int32 [S,k,2] = (x, y) in scene coordinates,
 *     point_clearance int32 [S,k], counts int32 [S], bbox int32 [S,4] in scene coordinates (INT_MAX,INT_MAX,-1,-1: never occurs).
 *   a round j = 0..k-1: dm_scene_point_select once per tile, in any order, then dm_scene_point_commit once.  Round j + 1 reads
 *     round j's committed points, so a scene costs k passes over its label raster.
 *   window: labels int32 [wh,ww] and clearance uint16 [wh,ww] = dm_label_clearance of THAT window, wh*ww < 2^31, whose first
 *     pixel is (oy, ox) of the scene.  Only the core rows cy0..cy1-1, columns cx0..cx1-1 of the window are candidates; the
 *     cores of a round's calls must partition the scene.  The window must reach (max_window + 1) / 2 pixels beyond the core
 *     on every side, clipped to the scene: then the window's clearance at a core pixel is the scene's (the cap equals that
 *     reach, and beyond a clipped side lies the outside of the scene).
 *   the key: bits 56..63 the score (<= cap <= 192), bits 8..55 2^48 - 1 - linear index, bits 0..7 the pixel's clearance, a
 *     passenger behind a unique position.  One unsigned 64-bit max per superpixel: largest score, then smallest scene linear
 *     index.  The commit reads position and clearance out of the key: it needs no raster and no tile resident.
 * dm_scene_point_init: best and counts to 0, bbox to the empty box; once, before round 0.
 * dm_scene_point_select: one tile's part of round `round`; round 0 also folds the core's pixels into bbox.
 * dm_scene_point_commit: every superpixel with a winner gets its next point; best is cleared for the next round.
 * dm_point_emit then runs unchanged on the scene's tables.  Every entry point validates before any launch, launches on
 * `stream`, never synchronises and never allocates. */
#define DM_SCENE_POINTS_MAX_PIXELS (1LL << 48)
int dm_scene_point_init(uint64_t *best, int32_t *counts, int32_t *bbox, int32_t S, void *stream);
int dm_scene_point_select(const int32_t *labels, const uint16_t *clearance, int32_t wh, int32_t ww, int32_t cy0, int32_t cy1,
                          int32_t cx0, int32_t cx1, int64_t oy, int64_t ox, int64_t scene_h, int64_t scene_w, int32_t S, int32_t k,
                          int32_t round, const int32_t *points, const int32_t *counts, uint64_t *best, int32_t *bbox, void *stream);
int dm_scene_point_commit(uint64_t *best, int64_t scene_h, int64_t scene_w, int32_t S, int32_t k, int32_t *points,
                          int32_t *point_clearance, int32_t *counts, void *stream);

/* ---- overlap of a label raster with a ground-truth raster: pair labels and partition scores (additive in ABI 6;
 * csrc/dm_truth.hip, DESIGN.md 3.5.3, rag.label_overlap / rag.pair_flags / Overlap.scores) ----------------------------------------
 * Replaces the `positive` / `negative` polygon-pair lists the reference reads from text files that were made outside the program
 * by comparing the over-segmentation with a ground-truth map (GenerateTrainPairData.py only counts their lines), and adds what
 * the reference lacks: a score of a PARTITION against a reference map.  The rule is this build's (restated in numpy in
 * tests/truth_ref.py).  All arithmetic is on integers; results are bit-exact.
 * The rule.  labels int32 [H,W]: region ids 0..S-1, ids outside [0,S) are ignored.  truth int32 [H,W]: object ids 0..G-1, any
 * other value means "unlabelled" and is counted under the pseudo-object G.  H*W < 2^31, G < 2^31, S*(G+1) < 2^62 (S and G are
 * passed as int64 so that the library, not an integer conversion in the binding, checks the bound).
 *   overlap table: n[s,g] = number of pixels with labels == s and truth column g, g in 0..G; sparse: keys s*(G+1)+g with int32
 *     counts, non-zero cells only, in ARBITRARY order (sort by key for a canonical list).
 *   row facts [S]: area[s] = sum over all G+1 columns (int64); owner[s] = the g < G with the largest n[s,g] >= 1, ties to the
 *     smallest g, -1 when s has no labelled pixel; owner_count[s] = n[s,owner[s]] or 0.  As the key
 *     (count << 32) | (0xFFFFFFFF - g) this is one unsigned 64-bit max per row.
 *   column facts [G]: size[g] = sum of n[s,g] over s (int64); cover[g] = max of n[s,g] over s (int32).
 *   pair flags: purity_pm in 0..1000; pure(s) iff owner[s] >= 0 and 1000*owner_count[s] >= purity_pm*area[s] (int64).  Edge (a,b):
 *     1 (merge) iff both pure and owner[a] == owner[b]; 0 iff both pure and the owners differ; -1 (ambiguous, not a training
 *     pair) otherwise, which includes any edge with an endpoint outside [0,S).
 *   summary int64 [8], over the labelled columns g < G only: n = sum n[s,g]; sum n[s,g]^2; sum_s r_s^2 with r_s = sum_{g<G} n[s,g];
 *     sum_g size[g]^2; sum_s owner_count[s]; sum_g cover[g]; number of rows with r_s > 0; number of columns with size > 0.
 *     Every sum is bounded by n^2 < 2^62.
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates.
 *
 * dm_label_overlap: one pass over both rasters (8 B per pixel).  table_keys / table_counts: scratch of 2^capacity_log2 entries
 *   (int64 / int32, 8 <= capacity_log2 <= 30); cell_keys / cell_counts: up to max_cells results; n_cells[0] = number found (may
 *   exceed max_cells: then the output is truncated); overflow[0] = 1 if the table was too small.  All outputs and scratch are
 *   (re)initialised by the call.
 * dm_overlap_reduce: row facts, column facts and summary from K cells in any order (K = 0: every fact is that of an empty table).
 *   Keys must be unique (fold duplicates first); entries with a key outside [0, S*(G+1)) or a count < 1 are skipped.
 *   Scratch: row_best uint64 [S], row_labelled int64 [S] (= r_s on return).  All outputs are (re)initialised by the call.
 * dm_pair_flags: flags int8 [E] for edges int32 [E,2] from the row facts. */
int dm_label_overlap(const int32_t *labels, const int32_t *truth, int32_t H, int32_t W, int64_t S, int64_t G, int64_t *table_keys,
                     int32_t *table_counts, int32_t capacity_log2, int64_t *cell_keys, int32_t *cell_counts, int32_t max_cells,
                     int32_t *n_cells, int32_t *overflow, void *stream);
int dm_overlap_reduce(const int64_t *cell_keys, const int32_t *cell_counts, int32_t K, int64_t S, int64_t G, uint64_t *row_best,
                      int64_t *row_labelled, int64_t *area, int32_t *owner, int32_t *owner_count, int64_t *size, int32_t *cover,
                      int64_t *summary, void *stream);
int dm_pair_flags(const int32_t *edges, int32_t E, const int64_t *area, const int32_t *owner, const int32_t *owner_count, int32_t S,
                  int32_t purity_pm, int8_t *flags, void *stream);

/* ---- boundary recall / precision of a label raster against a ground-truth raster at a pixel tolerance (additive in ABI 7;
 * csrc/dm_boundary.hip, DESIGN.md 3.5.17, rag.boundary_scores / MergeResult.boundary_scores / scene.boundary_scores) ------------
 * The region scores above say how well regions and objects overlap; these say where the partition's boundaries lie.  The rule is
 * this build's (restated in numpy in tests/boundary_ref.py).  All arithmetic is on integers; results are bit-exact.
 * The rule.  labels int32 [H,W]: region ids 0..S-1; truth int32 [H,W]: object ids 0..G-1; mapping (optional) int32 [S];
 * tolerance 0 <= d <= 64; H*W < 2^31.
 *   1. canonical value: v_L(p) = labels(p), or mapping[labels(p)] with a mapping, if 0 <= labels(p) < S, else -1 (a negative
 *      mapping entry is -1 as well); v_T(p) = truth(p) if 0 <= truth(p) < G, else -1 = unlabelled.  Two different out-of-range
 *      ids are therefore the same value.
 *   2. boundary pixel: b(p) = 1 iff the right neighbour (y, x+1) lies inside the raster and has another canonical value, or the
 *      lower neighbour (y+1, x) does.  The raster's frame is no boundary, and boundaries are one pixel thick (the 8-neighbour,
 *      frame-included bits of the clearance rule above are another rule: a two-pixel boundary would match itself at d = 0).
 *   3. match: m_X(p) = 1 iff some pixel q of the raster has b_X(q) = 1 and max(|dy|, |dx|) <= d.
 *   4. four counts over the pixels p of a box [y0,y1) x [x0,x1) (q may lie anywhere in the raster):
 *      n_truth_b = #{b_T(p)}, hit_truth = #{b_T(p) and m_L(p)}, n_label_b = #{b_L(p) and (v_T(p) >= 0 or m_T(p))},
 *      hit_label = #{b_L(p) and m_T(p)}: an unmatched region boundary in unlabelled territory is not held against the partition.
 *   recall = hit_truth / n_truth_b, precision = hit_label / n_label_b and F are the caller's.  Counts of disjoint boxes add.
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates.
 *
 * dm_boundary_bits: one read of a raster [H,W] with ids 0..n_ids-1 (mapping: int32 [n_ids] or NULL): edge uint64 [H * ceil(W/64)],
 *   bit x % 64 of word y * ceil(W/64) + x / 64 = b(y, x), bits behind x = W - 1 zero; valid (or NULL): the same layout, v >= 0.
 * dm_boundary_counts: counts int64 [4] += (n_truth_b, hit_truth, n_label_b, hit_label) of the box at tolerance d, from the bits
 *   of the labels and of the truth (zero counts before the first call; several boxes or tiles may add into the same four). */
#define DM_BOUNDARY_MAX_TOLERANCE 64
int dm_boundary_bits(const int32_t *raster, int32_t H, int32_t W, int32_t n_ids, const int32_t *mapping, uint64_t *edge,
                     uint64_t *valid, void *stream);
int dm_boundary_counts(const uint64_t *label_edge, const uint64_t *truth_edge, const uint64_t *truth_valid, int32_t H, int32_t W,
                       int32_t d, int32_t y0, int32_t y1, int32_t x0, int32_t x1, int64_t *counts, void *stream);

/* ---- SLIC superpixels from an image tile, 4-connected component labelling (additive in ABI 6; csrc/dm_slic.hip, DESIGN.md 3.5.4,
 * rag.slic / rag.connected_labels) ------------------------------------------------------------------------------------------------
 * Produces, on the device, the over-segmentation the reference reads from shapefiles written by external GIS software.  The
 * reference never defines it; the rule is this build's (restated in numpy in tests/slic_ref.py).  All arithmetic is on integers;
 * nothing depends on the order in which threads arrive; results are bit-exact.
 * The rule.  tile uint8 [bands,H,W], the first nb = min(bands, 4) bands are used; H*W < 2^31; 4 <= cell <= 256;
 * 0 <= compactness <= 255; iters >= 0; min_size >= 1.
 *   1. centres: gy = ceil(H / cell), gx = ceil(W / cell), K = gy*gx.  Centre c = j*gx + i starts at y = min(H-1, j*cell + cell/2),
 *      x = min(W-1, i*cell + cell/2) with the colour of the pixel there.  Positions and colours are integers.
 *   2. assignment: pixel (y, x) of grid cell (j, i) = (y / cell, x / cell) considers the up to 9 centres of the grid cells
 *      (j+dj, i+di), dj, di in -1..1, inside the grid, and takes the one with the smallest
 *        D = cell^2 * sum_b (p_b - c_b)^2 + compactness^2 * ((y - c_y)^2 + (x - c_x)^2);  ties go to the smaller centre id.
 *      A centre of cell J owns pixels of the cells J-1..J+1 only, so a pixel and a candidate are less than 3 cell apart on either
 *      axis and D <= cell^2 (nb 255^2 + 18 compactness^2): 32-bit arithmetic where that is below 2^32, 64-bit otherwise.
 *   3. update: a centre with n >= 1 pixels becomes the rounded mean (2 sum + n) / (2 n) of their y, x and every band; a centre
 *      without pixels stays.  The sequence is: assignment, then iters times (update, assignment).
 *   4. components: the assignment is split into 4-connected components of equal label, numbered 0..n-1 in the order of their
 *      first pixel in raster-scan order.
 *   5. absorption, in rounds: with areas and shared boundary lengths (pixel edges, as dm_rag_edges counts them) as they are at the
 *      start of the round, every region with area < min_size that has a neighbour picks the neighbour with the longest shared
 *      boundary, ties to the smaller id: one unsigned 64-bit max of (weight << 32) | (0xFFFFFFFF - neighbour) per region.  The
 *      picks are united (regions = connected components of the pick graph) and the regions renumbered by first pixel.  Rounds
 *      repeat until none picks.  The number of small regions at least halves per round.
 *   6. result: labels int32 [H,W] with ids 0..n-1, and n.
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates.
 *
 * dm_slic_iterate: steps 1-3, the whole loop without a readback.  centres int32 [K,6] = y, x, band 0..3 (the final centres on
 *   return), sums int64 [K,7] scratch, labels int32 [H,W] = the centre id of every pixel after the last assignment.
 * dm_connected_labels: step 4 for any int32 raster.  use_background != 0: pixels equal to `background` belong to no component
 *   and get -1.  Scratch: parent int32 [H*W], chunk_counts int32 [ceil(H*W / 4096) + 1].  labels int32 [H,W] (not the raster
 *   itself), n_labels[0] = the number of components.
 * dm_label_area: area int32 [S] = pixels of every id in [0,S) (cleared by the call); other ids are ignored.
 * dm_slic_absorb_pick: the picks of one round of step 5 over E >= 1 edges (a < b, as dm_rag_edges yields them): best uint64 [S]
 *   scratch, merge uint8 [E] = 1 iff one end of the edge picked the other, n_picked[0] = number of such edges.  All
 *   (re)initialised by the call.  dm_merge_round over `merge` unites the picks; dm_relabel_raster applies them. */
int dm_slic_iterate(const uint8_t *tile, int32_t bands, int32_t H, int32_t W, int32_t cell, int32_t compactness, int32_t iters,
                    int32_t *centres, int64_t *sums, int32_t *labels, void *stream);
int dm_connected_labels(const int32_t *raster, int32_t H, int32_t W, int32_t use_background, int32_t background, int32_t *parent,
                        int32_t *chunk_counts, int32_t *labels, int32_t *n_labels, void *stream);
int dm_label_area(const int32_t *labels, int32_t H, int32_t W, int32_t S, int32_t *area, void *stream);
int dm_slic_absorb_pick(const int32_t *edges, const int32_t *weights, int32_t E, const int32_t *area, int32_t S, int32_t min_size,
                        uint64_t *best, uint8_t *merge, int32_t *n_picked, void *stream);

/* ---- SLIC on a scene larger than one tile: superpixels that cross tile seams (additive in ABI 7; csrc/dm_scene_slic.hip,
 * csrc/dm_slic_pass.h, DESIGN.md 3.5.15, scene.slic_assign / scene.slic_labels) ------------------------------------------------------
 * The rule above on an H x W scene that is streamed through the device core by core (a core: h x w pixels whose first pixel is
 * (y0, x0) of the scene, uint8 [bands,h,w]); the result equals the tile form's on the whole scene bit for bit, whatever the cores.
 * The scene form of the rule.
 *   1. one table of K = ceil(H / cell) * ceil(W / cell) centres for the scene.  A centre starts at its scene position with the
 *      colour read from the core that holds that pixel: dm_scene_slic_init once per core, all cores before any dm_scene_slic_pass.
 *   2. a pixel's assignment depends on its colour, its scene position (y0 + y, x0 + x) and the up to 9 centres around its grid cell,
 *      all of them rows of the table: a core needs no halo and no neighbour's labels.  Centre ids are the scene's j*gx + i.
 *   3. the sums are integer adds, so the sums over the cores are the sums over the scene: per round dm_scene_slic_pass with `sums`
 *      for every core, in any order, then dm_scene_slic_update once; after the rounds dm_scene_slic_pass with `labels` for every
 *      core.  No readback inside the loop.
 *   4.-5. components and absorption are finished on the component graph (scene.slic_labels): tile-local components
 *      (dm_connected_labels) joined across a seam where the two facing pixels hold the same centre id, numbered by scene-wide first
 *      pixel; areas and shared boundary lengths add under a union, so the rounds of step 5 run on the folded graph
 *      (dm_slic_absorb_pick, dm_merge_round) and one dm_relabel_raster per core applies the composed mapping.
 * Limits, each checked before any launch: bands >= 1; H, W < 2^31 (int32); 0 <= y0, y0 + h <= H, 0 <= x0, x0 + w <= W; a core has
 * h*w < 2^31 pixels; 4 <= cell <= 256; K < 2^31; 0 <= compactness <= 255.  The sums are 64-bit: a centre owns at most (3 cell)^2
 * pixels.  On the graph (scene.slic_labels checks them): fewer than 2^31 provisional components and fewer than 2^31 edges in the
 * scene (dm_merge_round's and dm_slic_absorb_pick's int32 S and E); at most 2^25 components in one core (dm_rag_edges' table of 32
 * slots per label ends at 2^30); a shared boundary shorter than 2^31 pixel edges (int32 weights); areas are folded in 64 bits and
 * handed to dm_slic_absorb_pick clamped to 2^31 - 1, which `area < min_size` cannot tell from the area.  The pairs across the
 * seams are counted by the caller with one sort over the seam positions (a perimeter's worth): dm_seam_stitch's ids end at
 * 2^24, below the fragments a scene has before the absorption.
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates.
 *
 * dm_scene_slic_init: the centres whose start pixel lies in the core (int32 [K,6] rows = y, x, band 0..3 in scene coordinates) and
 *   their rows of sums int64 [K,7] (cleared).  Rows of other cores' centres are not touched.
 * dm_scene_slic_pass: one assignment pass over the core against the table.  sums != NULL: the core's pixels are added to the rows
 *   of the centres they take (n, sum y, sum x in scene coordinates, sum band 0..3).  labels != NULL: int32 [h,w] = the centre id of
 *   every pixel of the core.  Either may be NULL, not both.  16-byte strip loads and stores when w % 16 == 0 and core / labels are
 *   16-byte aligned, scalar otherwise; 32-bit distances where cell^2 (nb 255^2 + 18 compactness^2) < 2^32, 64-bit otherwise.
 * dm_scene_slic_update: step 3 over the K rows: rounded means into centres, sums cleared. */
int dm_scene_slic_init(const uint8_t *core, int32_t bands, int32_t h, int32_t w, int32_t y0, int32_t x0, int32_t H, int32_t W,
                       int32_t cell, int32_t *centres, int64_t *sums, void *stream);
int dm_scene_slic_pass(const uint8_t *core, int32_t bands, int32_t h, int32_t w, int32_t y0, int32_t x0, int32_t H, int32_t W,
                       int32_t cell, int32_t compactness, const int32_t *centres, int64_t *sums, int32_t *labels, void *stream);
int dm_scene_slic_update(int32_t K, int32_t *centres, int64_t *sums, void *stream);

/* ---- polygon rings and boundary arcs from a label raster (additive in ABI 6; csrc/dm_vector.hip, DESIGN.md 3.5.5,
 * rag.polygons / rag.boundary_arcs) ----------------------------------------------------------------------------------------------
 * Produces, on the device, the geometry the reference reads from shapefiles written by external GIS software (the polygon layer,
 * MyUtils1.py:79-114; one polyline per shared boundary with LEFT_FID / RIGHT_FID, MyUtils2.py:155-193).  The reference never
 * defines it; the rule is this build's (restated in numpy in tests/vector_ref.py).  All arithmetic is on integers; nothing depends
 * on the order in which threads arrive; results are bit-exact.
 * The rule.  labels int32 [H,W] with ids 0..S-1 (a label need not be connected; the caller checks the range), H*W <= 2^28.
 *   Pixel (x, y) covers [x, x+1] x [y, y+1]; corners are (x, y), 0 <= x <= W, 0 <= y <= H, y down.
 *   1. darts: a pixel has a dart on every side whose neighbour has another label or lies outside the raster; `other` is that
 *      label, -1 outside.  Side 0 (top) runs east from (x, y), 1 (right) south from (x+1, y), 2 (bottom) west from (x+1, y+1),
 *      3 (left) north from (x, y+1): the pixel lies on the dart's right.  dart id = 4 (y W + x) + side.
 *   2. successor of a dart of label l that ends at corner c, with the two pixels ahead of c seen along the dart: ahead-right is
 *      not l: side (side+1)&3 of the same pixel; else ahead-left is not l: the same side of the ahead-right pixel; else side
 *      (side+3)&3 of the ahead-left pixel.  Right turns first: labels that touch diagonally are not joined (4-connectivity).
 *      The successor map is a permutation of the darts.
 *   3. rings: a ring is a cycle, its head the smallest dart id, its label l.  A vertex dart is one whose predecessor has another
 *      side (the head is one).  The ring's vertices are the start corners of its vertex darts in cycle order from the head (not
 *      closed).  area2 = the shoelace sum over the ring, int64: positive for an outer ring, negative for a hole.  Rings are
 *      ordered by (label, head).
 *   4. arcs: a break dart is one whose predecessor has another `other`.  A ring without one is one closed arc from its head;
 *      otherwise an arc runs from a break dart to the last dart before the next.  Vertices: the start corner of the first dart,
 *      the start corners of the later vertex darts, the end corner of the last dart.  Kept iff other == -1 or other > l, with
 *      right = l, left = other; ordered by (right, left, id of the first dart).
 * Slots: darts are stored compacted, D of them, in tile order.  Every entry point validates before any launch, launches on
 * `stream`, never synchronises and never allocates; the caller reads back D, the round flags and the ring / arc counts, and sorts
 * and scans the ring and arc tables between the calls (rag._trace).
 *
 * dm_vector_count: mask uint8 [H,W] = the 4-bit side mask of every pixel; tile_off int32 [tiles+1] (tiles = ceil(H/64) ceil(W/64)) =
 *   exclusive scan of the darts per 64x64 tile, tile_off[tiles] = n_darts[0] = D.
 * dm_vector_emit: first_slot int32 [H,W]: slot(dart) = first_slot[pixel] + popcount(mask & ((1 << side) - 1)); dart int32 [D].
 * dm_vector_link: per slot next (successor slot), lab, other, flags uint8 (1 vertex dart, 2 break dart), key int64 = dart id << 32 | slot.
 * dm_vector_head_round: key_out[i] = min(key_in[i], key_in[jump_in[i]]), jump_out[i] = jump_in[jump_in[i]]; changed[0] = 1 iff a
 *   key changed (cleared by the call).  Start with jump_in = next; when changed stays 0, key & 0xffffffff is the slot of the ring's
 *   head.  The buffers of a round are distinct.
 * dm_vector_rank_init: sum int64 [D] = vertex flag << 32 | break flag, nxt int32 [D] = next, -1 in front of the head; the heads'
 *   ring_key int64 = label << 32 | head dart id and ring_slot, in arrival order (the caller sorts them), n_rings[0] = R <= D / 4.
 * dm_vector_rank_round: sum_out[i] = sum_in[i] + sum_in[nxt_in[i]], nxt_out[i] = nxt_in[nxt_in[i]]; changed[0] = 1 iff a nxt_out is
 *   not -1.  When it stays 0, sum is the count of vertex / break darts from the dart to the end of its cut cycle.
 * dm_vector_ring_emit: with ring_of_slot (ring index at every head slot), ring_ptr int64 [R+1] (scan of the rings' vertex counts,
 *   sum[head] >> 32) and arc_base int32 [R+1] (scan of max(1, break darts of the ring)): xy int32 [V,2], area2 int64 [R], and per arc
 *   of the unsorted arc table [n_arcs]: arc_first (dart id), arc_left, arc_right, arc_vstart (scratch), arc_count (vertices).
 * dm_vector_arc_emit: with arc_pos int32 [n_arcs] (row of the arc among the kept, sorted arcs, -1 = dropped) and arc_ptr int64 [A+1]:
 *   arc_xy int32 [Va,2]. */
typedef struct DmVectorTrace {
  const int32_t *dart, *next, *lab, *other;
  const uint8_t *flags;
  const int64_t *key, *sum;
  const int32_t *ring_of_slot;
  const int64_t *ring_ptr;
  const int32_t *arc_base;
  int32_t *xy;
  int64_t *area2;
  int32_t *arc_first, *arc_left, *arc_right, *arc_vstart, *arc_count;
  const int32_t *arc_pos;
  const int64_t *arc_ptr;
  int32_t *arc_xy;
  int32_t W, D, R, n_arcs;
} DmVectorTrace;
int dm_vector_count(const int32_t *labels, int32_t H, int32_t W, uint8_t *mask, int32_t *tile_off, int32_t *n_darts, void *stream);
int dm_vector_emit(const uint8_t *mask, const int32_t *tile_off, int32_t H, int32_t W, int32_t *first_slot, int32_t *dart, void *stream);
int dm_vector_link(const int32_t *labels, const uint8_t *mask, const int32_t *first_slot, const int32_t *dart, int32_t H, int32_t W,
                   int32_t D, int32_t *next, int32_t *lab, int32_t *other, uint8_t *flags, int64_t *key, void *stream);
int dm_vector_head_round(const int64_t *key_in, const int32_t *jump_in, int64_t *key_out, int32_t *jump_out, int32_t D, int32_t *changed,
                         void *stream);
int dm_vector_rank_init(const int64_t *key, const int32_t *next, const uint8_t *flags, const int32_t *lab, int32_t D, int64_t *sum,
                        int32_t *nxt, int64_t *ring_key, int32_t *ring_slot, int32_t *n_rings, int32_t max_rings, void *stream);
int dm_vector_rank_round(const int64_t *sum_in, const int32_t *nxt_in, int64_t *sum_out, int32_t *nxt_out, int32_t D, int32_t *changed,
                         void *stream);
int dm_vector_ring_emit(const DmVectorTrace *t, void *stream);
int dm_vector_arc_emit(const DmVectorTrace *t, void *stream);

/* ---- a scene's label raster traced across tile seams (additive in ABI 7; csrc/dm_scene_vector.hip, DESIGN.md 3.5.10,
 * scene.trace_labels / SceneResult.trace) ---------------------------------------------------------------------------------------
 * The rule above, unchanged, for a raster L [scene_h, scene_w] that is read tile by tile and never resident: the result is,
 * array for array and bit for bit, what the one-raster calls give on the whole of L, whatever the tile size.  No new geometry
 * rule: rings are ordered by (label, smallest scene dart id), arcs by (right, left, first dart).
 * A tile is a core box of the scene and its window: the core grown by one pixel on every side and clipped to the scene (an apron
 * of the neighbours' labels).  Only the core's pixels own darts.  scene dart id = 4 ((y + oy) scene_w + (x + ox)) + side for the
 * window pixel (x, y) of a window whose first pixel is the scene's (ox, oy): int64.
 * Why the apron is enough: a core dart consults its own pixel, the ahead-right and the ahead-left pixel and the pixel across its
 * successor's side, all 8-neighbours of the core pixel; a window edge that is not a scene edge is never consulted for a core
 * dart, and one that is a scene edge is the raster's outside.
 *
 * dm_scene_vector_count: labels int32 [H,W] = the window (1 <= H*W <= 2^28), the core = [cy0,cy1) x [cx0,cx1) in window
 *   coordinates, at most one pixel from every window edge.  mask uint8 [H,W] = dm_vector_count's mask of the window; core_mask = the
 *   same inside the core, 0 outside; tile_off int32 [tiles+1] = exclusive scan of the CORE's darts per 64x64 tile of the window,
 *   tile_off[tiles] = n_darts[0] = D.  dm_vector_emit on (core_mask, tile_off) then leaves the core's window-local dart ids.
 * dm_scene_vector_link: for the D darts `dart` (window-local ids, as dm_vector_emit leaves them): id int64 = the scene dart id,
 *   succ int64 = the successor's scene dart id (its pixel may be an apron pixel: another tile's dart), lab, other, and succ_flags
 *   uint8 = the flags (1 vertex dart, 2 break dart) OF THE SUCCESSOR, which the caller scatters once it knows the successor's slot.
 *   1 <= D; the window lies in the scene; scene_h, scene_w < DM_SCENE_VECTOR_MAX_SIDE, scene_h * scene_w <=
 *   DM_SCENE_VECTOR_MAX_PIXELS (ids stay below 2^62).
 * The join is the caller's: concatenate the tiles' records, sort by id (slot order = id order), next = position of succ among the
 * sorted ids, flags[next] = succ_flags, key = slot << 32 | slot.  dm_vector_head_round / rank_init / rank_round then run
 * unchanged; rank_init's ring_key becomes label << 32 | head slot, which sorts as (label, smallest dart id).
 * dm_scene_vector_ring_emit / dm_scene_vector_arc_emit: dm_vector_ring_emit / dm_vector_arc_emit with dart int64 [D] (scene ids)
 *   and W int64 = scene_w; arc_first receives the first dart's SLOT (the caller's arc sort key: (left + 1) << 31 | slot).  Corners
 *   are int32, area2 the int64 integer atomic add.
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates. */
#define DM_SCENE_VECTOR_MAX_SIDE 2147483647LL        /* scene_h, scene_w < 2^31 - 1: every corner fits int32 */
#define DM_SCENE_VECTOR_MAX_PIXELS (1LL << 60)
typedef struct DmSceneVectorTrace {
  const int64_t *dart;
  const int32_t *next, *lab, *other;
  const uint8_t *flags;
  const int64_t *key, *sum;
  const int32_t *ring_of_slot;
  const int64_t *ring_ptr;
  const int32_t *arc_base;
  int32_t *xy;
  int64_t *area2;
  int32_t *arc_first, *arc_left, *arc_right, *arc_vstart, *arc_count;
  const int32_t *arc_pos;
  const int64_t *arc_ptr;
  int32_t *arc_xy;
  int64_t W;
  int32_t D, R, n_arcs;
} DmSceneVectorTrace;
int dm_scene_vector_count(const int32_t *labels, int32_t H, int32_t W, int32_t cy0, int32_t cy1, int32_t cx0, int32_t cx1, uint8_t *mask,
                          uint8_t *core_mask, int32_t *tile_off, int32_t *n_darts, void *stream);
int dm_scene_vector_link(const int32_t *labels, const uint8_t *mask, const int32_t *dart, int32_t H, int32_t W, int32_t D, int64_t oy,
                         int64_t ox, int64_t scene_h, int64_t scene_w, int64_t *id, int64_t *succ, int32_t *lab, int32_t *other,
                         uint8_t *succ_flags, void *stream);
int dm_scene_vector_ring_emit(const DmSceneVectorTrace *t, void *stream);
int dm_scene_vector_arc_emit(const DmSceneVectorTrace *t, void *stream);

/* ---- polygon rings rasterised into a label raster (additive in ABI 6; csrc/dm_rasterize.hip, DESIGN.md 3.5.6, rag.rasterize /
 * rag.labels_from_shapefile) ------------------------------------------------------------------------------------------------------
 * The inverse of the tracing above, for ANY polygon: the step from the polygon layer the reference's users have (superpixels
 * written by external GIS software, digitised ground truth) to the label raster every raster pass here starts from.  The rule is
 * this build's (restated in numpy in tests/rasterize_ref.py).  All arithmetic is on integers; nothing depends on the order in which
 * threads arrive; results are bit-exact.
 * The rule.
 *   coordinates: pixel-corner space as DmVectorTrace.xy uses it, x right, y down; pixel (c, r) covers [c, c+1] x [r, r+1], its
 *     centre is (c + 1/2, r + 1/2).
 *   quantisation: a float64 coordinate v becomes the int32 q = floor(v * DM_RASTERIZE_SUBPIXEL + 0.5): 8 sub-pixel bits.
 *     |v| <= 2^20 pixels (NaN and inf are refused), so |q| <= 2^28 and every product below stays under 2^60.  An integer corner x is
 *     256 x exactly.  The entry points take the quantised int32 coordinates.
 *   rings: a ring is always closed, the last vertex joins the first.  A repeated closing vertex (as shapefiles store it) is a
 *     zero-length edge that contributes nothing.  A ring that encloses nothing (fewer than 3 vertices, collinear vertices, zero
 *     area) contributes nothing, by the parity rule itself, and is not an error.  Vertices may lie outside the raster.
 *   crossings: an edge with ends (x0, y0), (x1, y1); y0 == y1 contributes nothing.  Otherwise the ends are swapped so that y0 < y1,
 *     dy = y1 - y0.  The edge crosses pixel row r iff y0 <= 256 r + 128 < y1 (half-open: a vertex on a centre row counts once).
 *     There, with Yc = 256 r + 128, num = x0 dy + (Yc - y0) (x1 - x0); the crossing is at X = num / dy.  Column c is right of it
 *     iff 256 c + 128 >= X, i.e. (256 c + 128) dy >= num: the event's column is cx = ceil((num - 128 dy) / (256 dy)), exact
 *     integer ceiling division, clamped to [0, W].  Rows outside [0, H) give no event.
 *   inside: pixel (c, r) belongs to label l iff the number of events of ALL rings of l in row r with cx <= c is odd (even-odd: holes
 *     need no flag, the doubly covered part of a self-intersecting ring is left out).  Polygons that share an edge partition the
 *     pixels along it: no gap, no double claim.
 *   output: int32 [H,W]; a pixel inside no label holds `fill` < 0; labels are 0 .. 2^31 - 2; a pixel inside several labels gets the
 *     greatest (integer max into a raster pre-set to `fill`).
 * Closed rings give every (label, row) an even number of events, so in the sorted keys events 2j and 2j+1 share (label, row) and
 * bound one span of the label's pixels.  Every entry point validates before any launch, launches on `stream`, never synchronises
 * and never allocates; the caller scans the counts, reads back N and sorts the keys between the calls (rag.rasterize).
 *
 * dm_rasterize_count: xy int32 [V,2] quantised, ring_ptr int64 [R+1] non-decreasing from 0 to V, vert_ring int32 [V] = the ring of
 *   every vertex.  Edge v runs from vertex v to its successor within its ring.  count int32 [V] = the events of edge v.
 * dm_rasterize_emit: scan int64 [V+1] = exclusive scan of count, N = scan[V] <= 2^30.  One thread per event: keys int64 [N],
 *   key = (label H + row) (W + 1) + cx with label = ring_label[ring] in [0, n_labels); n_labels H (W + 1) < 2^63.  An event whose
 *   edge the tables do not hold gets key -1.
 * dm_rasterize_fill: keys int64 [N] SORTED, N even (N = 0: keys may be NULL).  out int32 [H,W] is pre-set to fill < 0, then every
 *   pair (2j, 2j+1) writes max(label) over columns [cx of 2j, cx of 2j+1) of its row.  error[0] = 1 iff a pair's keys disagree in
 *   (label, row), a key is negative or a label exceeds 2^31 - 2 (cleared by the call); such a pair writes nothing. */
#define DM_RASTERIZE_SUBPIXEL 256
int dm_rasterize_count(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, int32_t V, int32_t R, int32_t H, int32_t W,
                       int32_t *count, void *stream);
int dm_rasterize_emit(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, const int32_t *ring_label, const int64_t *scan,
                      int32_t V, int32_t R, int64_t N, int32_t H, int32_t W, int64_t n_labels, int64_t *keys, void *stream);
int dm_rasterize_fill(const int64_t *keys, int64_t N, int32_t H, int32_t W, int32_t fill, int32_t *out, int32_t *error, void *stream);

/* ---- the same rule on a scene: a band of rows, a window of columns (additive in ABI 7; csrc/dm_scene_rasterize.hip, DESIGN.md
 * 3.5.16, scene.RingSource / scene.rasterize_rings; restated in numpy in tests/scene_rasterize_ref.py) ----------------------------
 * H x W is the SCENE, H, W < 2^31, and H W may be 2^31 or more: no raster of it is ever built.  The rule above is unchanged; what
 * changes is which rows an event pass covers and which columns a fill writes.
 *   band: the pixel rows [r0, r1), 0 <= r0 < r1 <= H.  An edge has an event in row r of the band iff r0 <= r < r1 and
 *     y0 <= 256 r + 128 < y1 (half-open at the band's first and last row as everywhere); cx as above, clamped to [0, W] SCENE-wide.
 *   key: (label (r1 - r0) + (r - r0)) (W + 1) + cx, with n_labels (r1 - r0) (W + 1) < 2^63; at most 2^30 events per band.  It does
 *     not depend on any window: one sort of a band's keys serves every window of that band.
 *   window: the columns [x0, x1), 0 <= x0 < x1 <= W, (r1 - r0) (x1 - x0) < 2^31.  out int32 [r1 - r0, x1 - x0] is pre-set to fill
 *     < 0, then every pair (2j, 2j+1) of the sorted keys writes max(label) over the columns [cx of 2j, cx of 2j+1) that lie in
 *     [x0, x1), at (r - r0, c - x0).  A crossing left of the window is clamped to no less than 0 <= x0, so it still opens a span that
 *     reaches into the window: the parity inside the window is the scene's.  Hence out equals rows [r0, r1), columns [x0, x1) of
 *     the whole raster wherever that exists, and always equals the rule applied to the rings translated by (-256 x0, -256 r0) on a
 *     raster (r1 - r0) x (x1 - x0): translation by whole pixels is exact in every formula above.
 *   error[0] = 1 iff ANY pair of the band disagrees in (label, row), has a negative key or a label above 2^31 - 2, whether or not its
 *     span meets the window (cleared by the call).
 * dm_rasterize_count_rows / dm_rasterize_emit_rows: dm_rasterize_count / _emit on the band; the other arguments as there.
 * dm_rasterize_fill_window: keys int64 [N] SORTED keys of the band [r0, r1), N even (N = 0: keys may be NULL). */
int dm_rasterize_count_rows(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, int32_t V, int32_t R, int32_t H, int32_t W,
                            int32_t r0, int32_t r1, int32_t *count, void *stream);
int dm_rasterize_emit_rows(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, const int32_t *ring_label,
                           const int64_t *scan, int32_t V, int32_t R, int64_t N, int32_t H, int32_t W, int32_t r0, int32_t r1,
                           int64_t n_labels, int64_t *keys, void *stream);
int dm_rasterize_fill_window(const int64_t *keys, int64_t N, int32_t H, int32_t W, int32_t r0, int32_t r1, int32_t x0, int32_t x1,
                             int32_t fill, int32_t *out, int32_t *error, void *stream);

/* ---- shared-boundary Douglas-Peucker on the traced rings and arcs (additive in ABI 6; csrc/dm_simplify.hip, DESIGN.md 3.5.7,
 * rag.simplify) ----------------------------------------------------------------------------------------------------------------
 * The tracing above leaves a pixel staircase.  Simplified per polygon, two neighbours would treat their common boundary
 * differently and leave slivers and overlaps; here every stretch of boundary is simplified once, as the arc that stores it, and
 * both neighbours see the result.  The rule is this build's (restated in numpy / Python ints in tests/simplify_ref.py).  All
 * arithmetic is on integers; nothing depends on the order in which threads arrive or segments are split; results are bit-exact.
 * The rule.  labels int32 [H,W], 1 <= H, W <= DM_SIMPLIFY_MAX_SIDE (so every |cross| below is under 2^31); corners as above.
 *   nodes: a corner (x, y), 0 <= x <= W, 0 <= y <= H, is a node iff at least three of its four unit grid edges are boundary
 *     edges (two different labels across; the outside of the raster counts as label -1), or it is one of the four raster corners.
 *     Nodes are never removed.  Every other corner on a boundary has exactly two boundary edges, so exactly one chain passes
 *     through it, once: a keep flag per corner is single-valued.
 *   chains: an arc of the tracing is cut at every vertex that is a node; an open arc also at its two ends (they are nodes: an arc
 *     ends where the label across changes).  The kept arc of a pair comes from the smaller label's ring and can run through a
 *     corner with four boundary edges unbroken: it is cut there.  A closed arc (first vertex == last) is the cyclic sequence of
 *     its vertices without the repeated end, and without its stored start when that is no node and lies inside a straight run (a
 *     hole's head dart need not be a vertex dart).  With no node among them the arc has no natural ends: its one chain begins and
 *     ends at the vertex smallest in (y, x), which is kept.
 *   Douglas-Peucker on a chain v[0..n-1]; the two ends are kept.  For a segment (i, j) with j > i + 1: d_k =
 *     |cross(v[j] - v[i], v[k] - v[i])| if v[i] != v[j], else |v[k] - v[i]|^2 (a closed chain's first split); k* = the arg-max of
 *     d_k over i < k < j, ties to the smallest k.  The tolerance t in pixels is quantised as rasterize quantises coordinates:
 *     q = floor(256 t + 0.5), 0 <= q <= DM_SIMPLIFY_MAX_Q.  k* is kept, and both halves (i, k*), (k*, j) are split further, iff
 *     65536 d^2 > q^2 |v[j] - v[i]|^2 (distinct ends) or 65536 d > q^2 (coinciding ends): both exact in 128 bits.
 *   keep uint8 [(H+1)(W+1)], corner (x, y) at y (W+1) + x: 2 for a node, 1 for a kept chain vertex, 0 otherwise.
 *   arcs out: the same arcs in the same order, each with its kept vertices in stored order; a closed arc begins at its first kept
 *     vertex (a stored start that is not kept is rotated away) and repeats that vertex at its end.
 *   rings out: the same rings in the same order; a ring becomes the kept corners met when walking from each of its vertices to
 *     the next, one unit step at a time.  The walk inserts the nodes that sit on a straight run of the ring (T-junctions, where a
 *     neighbour's chain ends): without them the neighbours would no longer share vertices.  area2 is the shoelace sum again; a
 *     ring left with fewer than three vertices or zero area is still there, with area2 == 0.
 * Shared boundaries stay shared and nodes stay put.  Two different chains may cross, at any tolerance above 0, as with any plain
 * Douglas-Peucker; the entries below (dm_simplify_topology_*) detect and repair it.  Every entry point validates before any launch, launches on `stream`, never synchronises
 * and never allocates; the caller scans the counts and reads back the vertex totals between count and emit (rag.simplify).
 *
 * dm_simplify_nodes: keep = 2 at the nodes, 0 elsewhere (every entry is written).
 * dm_simplify_chains: arc_xy int32 [Va,2], arc_ptr int64 [A+1] as DmVectorTrace leaves them, q as above; keep from
 *   dm_simplify_nodes gets its 1s.  One wavefront per arc; stack int64 [Va] is its workspace, laid out by arc_ptr: a depth-first
 *   walk that pushes one half of every split never holds more entries than the chain has interior vertices.  An arc with a vertex
 *   outside the raster is left alone.
 * dm_simplify_arc_count: count int32 [A] = the kept vertices of every arc (with the repeated end of a closed arc).
 * dm_simplify_arc_emit: new_ptr int64 [A+1] = the exclusive scan of count, Vn = new_ptr[A]; out_xy int32 [Vn,2].
 * dm_simplify_ring_count: xy int32 [V,2], ring_ptr int64 [R+1], vert_ring int32 [V] = the ring of every vertex; count int32 [V] =
 *   the kept corners on the unit steps from vertex v (included) to its successor within its ring (excluded).
 * dm_simplify_ring_emit: scan int64 [V+1] = the exclusive scan of count, Vn = scan[V], new_ring_ptr int64 [R+1] = scan at
 *   ring_ptr; out_xy int32 [Vn,2], area2 int64 [R] (cleared, then summed with integer atomics). */
#define DM_SIMPLIFY_MAX_SIDE 32768
#define DM_SIMPLIFY_MAX_Q (1 << 20)
int dm_simplify_nodes(const int32_t *labels, int32_t H, int32_t W, uint8_t *keep, void *stream);
int dm_simplify_chains(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int32_t H, int32_t W, int32_t q, uint8_t *keep,
                       int64_t *stack, void *stream);
int dm_simplify_arc_count(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int32_t H, int32_t W, const uint8_t *keep,
                          int32_t *count, void *stream);
int dm_simplify_arc_emit(const int32_t *arc_xy, const int64_t *arc_ptr, const int64_t *new_ptr, int32_t A, int64_t Va, int64_t Vn, int32_t H,
                         int32_t W, const uint8_t *keep, int32_t *out_xy, void *stream);
int dm_simplify_ring_count(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, int32_t V, int32_t R, int32_t H, int32_t W,
                           const uint8_t *keep, int32_t *count, void *stream);
int dm_simplify_ring_emit(const int32_t *xy, const int64_t *ring_ptr, const int32_t *vert_ring, const int64_t *scan, const int64_t *new_ring_ptr,
                          int32_t V, int32_t R, int64_t Vn, int32_t H, int32_t W, const uint8_t *keep, int32_t *out_xy, int64_t *area2,
                          void *stream);

/* ---- topology-safe simplification: find and repair boundary conflicts (additive in ABI 7; csrc/dm_simplify_topology.hip,
 * DESIGN.md 3.5.12, rag.simplify(topology=True) / rag.simplify_conflicts) ---------------------------------------------------------
 * Plain Douglas-Peucker moves every chain on its own: islands collapse to a point, two boundaries land on each other, a boundary
 * swings over a neighbour's corner.  The arcs are stored once per shared boundary and every vertex is an integer, so the damage is
 * found exactly and repaired for both neighbours at once, only by keeping vertices the rule above had dropped.  Restated in numpy /
 * Python ints in tests/simplify_topology_ref.py; integers only; nothing depends on the order in which anything is tested.
 * The rule.  orient(a, b, c) = (b.x - a.x)(c.y - a.y) - (b.y - a.y)(c.x - a.x): coordinates are at most 32768, below 2^31.
 *   segments: for the current keep, every chain is the sequence of its kept vertices; a segment is two consecutive kept vertices
 *     (v[i], v[j]) of one chain, its interior vertices are v[i+1 .. j-1] of the traced chain.  The frame arcs (left == -1) are
 *     segments like any other.  Order: by arc, then along the arc as dm_simplify_arc_emit writes it (segment s of an arc joins
 *     vertices s and s + 1 of the simplified arc).
 *   fixed points: every node (keep == 2) and the anchor of every closed arc without a node.  They never move.
 *   kind, a bit set per segment.
 *     bit 1, meets: the segment is degenerate (v[i] == v[j]: a closed chain collapsed to its start), or it shares with another
 *       segment of the scene a point that is not an end of both.  Between two non-degenerate segments (A, B), (C, D): {A, B} ==
 *       {C, D}; or a proper crossing (orient(A,B,C), orient(A,B,D) of strictly opposite signs and so orient(C,D,A),
 *       orient(C,D,B)); or an end of one on the other (orient == 0, inside the bounding box) that is not also an end of that
 *       other.  Both segments of a meeting pair are flagged; degenerate segments take no part in pair tests.
 *     bit 2, jumps: the segment has interior vertices and some fixed point p other than v[i], v[j] is inside the polygon v[i],
 *       v[i+1], .., v[j] closed by the segment, by the even-odd rule, half-open in y: the edges (u, w) with (u.y <= p.y) !=
 *       (w.y <= p.y) and (w.y > u.y and orient(u,w,p) > 0, or w.y < u.y and orient(u,w,p) < 0) are odd in number.
 *   repair, in rounds: a round computes the kinds of all segments of the current keep; every flagged segment with interior
 *     vertices has its arg-max k* kept (d_k and the ties as above) and both halves (i, k*), (k*, j) simplified by the ordinary
 *     rule at the same q; flagged segments without interior vertices are left alone.  Rounds repeat until no segment is flagged;
 *     then count and emit run once on the final keep.  The traced arcs are conflict-free and every round keeps at least one more
 *     vertex, so this ends; the caller gives up past its round limit.
 * The search structure: a uniform grid of cells of 2^DM_SIMPLIFY_TOPOLOGY_CELL_LOG2 corners a side, (H >> log2) + 1 rows of
 * (W >> log2) + 1; a point is in the cell of its coordinates >> log2, a segment in every cell one of its points is in (walked
 * along the segment, not over its box).  Per-cell lists by count, the caller's scan, fill.
 *
 * One struct for all entries; every entry validates before any launch, launches on `stream`, never synchronises, never allocates.
 *   point_count: clears point_count / point_fill, then point_count[cell] = the fixed points of the cell, one per arc vertex that
 *     is a node (a node is counted once for every arc that passes through or ends at it) or anchor.  keep after dm_simplify_chains.
 *   point_fill: point_ptr = the exclusive scan of point_count (at most Va in all); point_xy gets the points by cell.
 *   segments: clears cell_count / cell_fill / status; new_ptr = the exclusive scan of dm_simplify_arc_count on the current keep;
 *     seg slot e = (2 arc + skip, position in the arc as dm_simplify_chains sees it, x, y) of simplified vertex e.
 *   bin_count: kind[e] = 1 for a degenerate segment, else 0; cell_count[cell] = the other segments passing through the cell.
 *   bin_fill: cell_ptr = the exclusive scan of cell_count; cell_seg [cap] gets the slots by cell; status[2] = the entries needed
 *     (when above cap the lists are cut short: repeat the round with a larger cap; refine then keeps nothing).
 *   pairs: kind |= 1.   jumps: kind |= 2.
 *   refine: status[0] = flagged segments, status[1] = those with interior vertices; apply != 0: every one of those is split as
 *     the rule says.  stack int64 [2 Va]: segment (i, j) of an arc owns the j - i entries from 2 arc_ptr[arc] + i. */
#define DM_SIMPLIFY_TOPOLOGY_CELL_LOG2 5
typedef struct DmSimplifyTopology {
  const int32_t *arc_xy;          /* [Va,2] the traced arcs */
  const int64_t *arc_ptr;         /* [A+1] */
  const int64_t *new_ptr;         /* [A+1] */
  uint8_t *keep;                  /* [(H+1)(W+1)] */
  int32_t *point_count, *point_fill; /* [cells] */
  const int64_t *point_ptr;       /* [cells+1] */
  int32_t *point_xy;              /* [Va,2] */
  int32_t *seg;                   /* [Va,4], 16-byte aligned */
  int32_t *kind;                  /* [Va] */
  int32_t *cell_count, *cell_fill; /* [cells] */
  const int64_t *cell_ptr;        /* [cells+1] */
  int32_t *cell_seg;              /* [cap] */
  int64_t *stack;                 /* [2 Va] */
  int32_t *status;                /* [4] */
  int64_t Va, cap;
  int32_t A, H, W, q;
} DmSimplifyTopology;
int dm_simplify_topology_point_count(const DmSimplifyTopology *t, void *stream);
int dm_simplify_topology_point_fill(const DmSimplifyTopology *t, void *stream);
int dm_simplify_topology_segments(const DmSimplifyTopology *t, void *stream);
int dm_simplify_topology_bin_count(const DmSimplifyTopology *t, void *stream);
int dm_simplify_topology_bin_fill(const DmSimplifyTopology *t, void *stream);
int dm_simplify_topology_pairs(const DmSimplifyTopology *t, void *stream);
int dm_simplify_topology_jumps(const DmSimplifyTopology *t, void *stream);
int dm_simplify_topology_refine(const DmSimplifyTopology *t, int32_t apply, void *stream);

/* ---- shared-boundary Douglas-Peucker on a scene's rings and arcs across tile seams (additive in ABI 7;
 * csrc/dm_scene_simplify.hip, DESIGN.md 3.5.11, scene.simplify_labels / SceneResult.simplified) -----------------------------------
 * The rule above, unchanged, for a raster L [scene_h, scene_w] that is read tile by tile and never resident: the result is, array
 * for array and bit for bit, what the one-raster calls give on the whole of L, whatever the tile size.  No new geometry rule, only
 * a sparse form of `keep`, which as a raster would take (scene_h + 1)(scene_w + 1) bytes and 64-bit corner ids.  It rests on three
 * facts about the rule (asserted in tests/test_scene_simplify_host.py):
 *   1. a corner with keep == 1 is a stored vertex of exactly one arc, and occurs there once among the arc's positions below len;
 *   2. a node that lies on an arc is a stored vertex of that arc: the chain pass needs keep only at arc vertices;
 *   3. on the straight run of a ring from vertex v to its successor the kept corners are v itself, if kept, and exactly the nodes
 *      strictly inside the run (the T-junctions).
 * The sparse form: scene corner id = y (scene_w + 1) + x, int64.
 *   node_row int64 [n_nodes]: the ids of the scene's nodes, ascending; node_col int64 [n_nodes]: x (scene_h + 1) + y of the same
 *     nodes, ascending.  A scene has at least its four corners and fewer than 2^31 nodes.
 *   arc_keep uint8 [Va]: one byte per stored arc vertex, 2 where the vertex's corner is in node_row, else 0 (the caller's); the
 *     chain pass writes its 1s by position, arc_keep[first + skip + p mod len].
 *   kept_row int64 [n_kept]: ascending, the ids of the nodes and of the arc vertices with arc_keep == 1.  A ring vertex is kept iff
 *     it is found there; the nodes inside a run are one range of node_row (horizontal run) or node_col (vertical run).
 * Arithmetic limit: the rule's products need |cross| < 2^31 within a chain.  Differences are taken from v[i], so this is a limit
 * per arc: its bounding box at most DM_SIMPLIFY_MAX_SIDE on each side.  An arc beyond it is left alone by the chain pass, as is an
 * arc with a vertex outside the scene; the caller checks the extents and raises (scene.simplify_labels).
 * Every entry point validates before any launch, launches on `stream`, never synchronises and never allocates.
 *
 * dm_scene_simplify_node_count / node_emit: labels int32 [H,W] = the window dm_scene_vector_count reads, the core = [cy0,cy1) x
 *   [cx0,cx1) in window coordinates, the window's first pixel at (ox, oy) of the scene.  The core may touch a window edge only where
 *   that is the scene's edge.  Scene corner (X, Y), 0 <= X <= scene_w, 0 <= Y <= scene_h, belongs to the core that holds pixel
 *   (min(X, scene_w - 1), min(Y, scene_h - 1)).  The node rule is dm_simplify_nodes's: at least three of the four unit edges are
 *   boundary edges, or a scene corner; outside the SCENE is -1.  tile_off int32 [blocks+1], blocks = ceil((H+1)/64) ceil((W+1)/64):
 *   the exclusive scan of the owned nodes per 64x64 block of window corners, tile_off[blocks] = n_nodes[0] = N.  node_emit writes
 *   node int64 [N], the scene corner ids, in no particular order (the caller concatenates the tiles and sorts).
 * dm_scene_simplify_chains / arc_count / arc_emit: dm_simplify_chains / arc_count / arc_emit with arc_keep in the place of keep;
 *   2 <= Va < 2^31.  The anchor of a closed arc without a node is the vertex smallest in (y, x), by a wave minimum of the 64-bit
 *   corner id and then of the position among the lanes that hold it.
 * dm_scene_simplify_ring_count: one thread per ring vertex; count int32 [V] = (v kept) + the nodes strictly inside the run to its
 *   successor: three binary searches, O(log n_nodes) whatever the run's length.  status int32 [1] is cleared, then set to 1 where a
 *   list shows itself unsorted (a range that ends before it begins or holds more nodes than the run has inner corners).  No index
 *   is followed unchecked: every search stays inside its list, sorted or not.  The detection is best effort, not a test of
 *   sortedness: the host cannot see a device list without a synchronisation, so the entry returns DM_OK and a swap that leaves
 *   every searched range consistent goes unseen.  The caller sorts the lists (scene.simplify_labels does).
 * dm_scene_simplify_ring_emit: scan / new_ring_ptr / Vn / out_xy / area2 as dm_simplify_ring_emit takes them; the nodes of a run
 *   are emitted in the walk's direction; an entry outside its run's id range sets status (never cleared here) and ends the run.
 *   scene.simplify_labels reads status once, after ring_count; what ring_emit adds is for a direct caller of the entries to read.
 *   A shoelace term is below 2^63 and area2 at most 2 scene_h scene_w <= 2^61. */
typedef struct DmSceneSimplifyRings {
  const int32_t *xy;              /* [V,2] ring vertices in scene coordinates */
  const int64_t *ring_ptr;        /* [R+1] */
  const int32_t *vert_ring;       /* [V] */
  const int64_t *node_row, *node_col, *kept_row;
  int32_t *status;                /* [1] */
  int64_t n_nodes, n_kept, scene_h, scene_w;
  int32_t V, R;
} DmSceneSimplifyRings;
int dm_scene_simplify_node_count(const int32_t *labels, int32_t H, int32_t W, int32_t cy0, int32_t cy1, int32_t cx0, int32_t cx1, int64_t oy,
                                 int64_t ox, int64_t scene_h, int64_t scene_w, int32_t *tile_off, int32_t *n_nodes, void *stream);
int dm_scene_simplify_node_emit(const int32_t *labels, int32_t H, int32_t W, int32_t cy0, int32_t cy1, int32_t cx0, int32_t cx1, int64_t oy,
                                int64_t ox, int64_t scene_h, int64_t scene_w, const int32_t *tile_off, int32_t N, int64_t *node, void *stream);
int dm_scene_simplify_chains(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int64_t scene_h, int64_t scene_w, int32_t q,
                             uint8_t *arc_keep, int64_t *stack, void *stream);
int dm_scene_simplify_arc_count(const int32_t *arc_xy, const int64_t *arc_ptr, int32_t A, int64_t Va, int64_t scene_h, int64_t scene_w,
                                const uint8_t *arc_keep, int32_t *count, void *stream);
int dm_scene_simplify_arc_emit(const int32_t *arc_xy, const int64_t *arc_ptr, const int64_t *new_ptr, int32_t A, int64_t Va, int64_t Vn,
                               int64_t scene_h, int64_t scene_w, const uint8_t *arc_keep, int32_t *out_xy, void *stream);
int dm_scene_simplify_ring_count(const DmSceneSimplifyRings *t, int32_t *count, void *stream);
int dm_scene_simplify_ring_emit(const DmSceneSimplifyRings *t, const int64_t *scan, const int64_t *new_ring_ptr, int64_t Vn, int32_t *out_xy,
                                int64_t *area2, void *stream);

/* ---- topology-safe simplification of a scene (additive in ABI 7; csrc/dm_scene_simplify_topology.hip, DESIGN.md 3.5.13,
 * scene.simplify_labels_topology / scene.simplify_conflicts) --------------------------------------------------------------
 * The rule and the repair rounds of dm_simplify_topology_* above, unchanged, on a scene's arcs: the result is, array for array and
 * bit for bit, what the one-raster entries give on the whole raster.  The same kernels (csrc/dm_simplify_topology_kernels.h) in a
 * second form; the struct is DmSimplifyTopology with three differences:
 *   arc_keep uint8 [Va] in the place of keep: one byte per stored arc vertex as dm_scene_simplify_chains leaves it (2 node, 1 kept,
 *     0 dropped); a vertex's flag is found by its position in its arc, and refine writes its 1s there.  The caller builds kept_row
 *     from it after the last round.
 *   H, W are the scene's sides, 1 <= H, W < 2^31 - 1.
 *   cell_log2: the grid has cells of 2^cell_log2 corners a side, (H >> cell_log2) + 1 rows of (W >> cell_log2) + 1, and must have at
 *     most DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELLS of them (the product is formed in 64 bits); 5 <= cell_log2 <= 24.  The flags are
 *     ORs over all pairs that share a cell, and a segment is in the cell of every one of its points, so two segments that share a
 *     point share a cell at any cell side: the result does not depend on cell_log2.  Cell ids are int.
 * Arithmetic.  Coordinates are int32 in [0, 2^31 - 2]: every difference of two fits an int, every product of two differences is
 * below 2^62 and every orient below 2^63, so no entry overflows whatever the tables hold.  Within a chain the rule needs
 * |cross| < 2^31 (refine's arg-max key is d << 32 | ~(k - i)): the arc-extent limit of dm_scene_simplify_chains, a bounding box of
 * at most DM_SIMPLIFY_MAX_SIDE on each side.  An arc beyond it, or with a vertex outside the scene, has no fixed points; a
 * sub-chain beyond it is not tested for jumps and not refined: what the chain pass refuses stays refused, and the caller raises
 * before any of it (scene.simplify_labels).  Between two segments that share a cell, or a fixed point inside a sub-chain's box, one
 * factor of each product is such an extent and the other a difference below 2^32: every orient term met is below 2^48.
 * Sizes: 1 <= A < 2^30 (the table's tag is 2 arc + skip in an int), 2 <= Va <= 2^30, 0 <= q <= 2^20, 1 <= cap < 2^31.  Every entry
 * validates before any launch (DM_ERR_BAD_SHAPE), launches on `stream`, never synchronises, never allocates; every slot, arc,
 * position, cell range and point range is checked before it is followed.  The entries do what their namesakes above do;
 * `segments` takes new_ptr = the exclusive scan of dm_scene_simplify_arc_count on the current arc_keep. */
#define DM_SCENE_SIMPLIFY_TOPOLOGY_MIN_CELL_LOG2 5
#define DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELL_LOG2 24
#define DM_SCENE_SIMPLIFY_TOPOLOGY_MAX_CELLS (1LL << 22)
typedef struct DmSceneSimplifyTopology {
  const int32_t *arc_xy;          /* [Va,2] the traced arcs, scene coordinates */
  const int64_t *arc_ptr;         /* [A+1] */
  const int64_t *new_ptr;         /* [A+1] */
  uint8_t *arc_keep;              /* [Va] */
  int32_t *point_count, *point_fill; /* [cells] */
  const int64_t *point_ptr;       /* [cells+1] */
  int32_t *point_xy;              /* [Va,2] */
  int32_t *seg;                   /* [Va,4], 16-byte aligned */
  int32_t *kind;                  /* [Va] */
  int32_t *cell_count, *cell_fill; /* [cells] */
  const int64_t *cell_ptr;        /* [cells+1] */
  int32_t *cell_seg;              /* [cap] */
  int64_t *stack;                 /* [2 Va] */
  int32_t *status;                /* [4] */
  int64_t Va, cap;
  int32_t A, H, W, q, cell_log2;
} DmSceneSimplifyTopology;
int dm_scene_simplify_topology_point_count(const DmSceneSimplifyTopology *t, void *stream);
int dm_scene_simplify_topology_point_fill(const DmSceneSimplifyTopology *t, void *stream);
int dm_scene_simplify_topology_segments(const DmSceneSimplifyTopology *t, void *stream);
int dm_scene_simplify_topology_bin_count(const DmSceneSimplifyTopology *t, void *stream);
int dm_scene_simplify_topology_bin_fill(const DmSceneSimplifyTopology *t, void *stream);
int dm_scene_simplify_topology_pairs(const DmSceneSimplifyTopology *t, void *stream);
int dm_scene_simplify_topology_jumps(const DmSceneSimplifyTopology *t, void *stream);
int dm_scene_simplify_topology_refine(const DmSceneSimplifyTopology *t, int32_t apply, void *stream);

/* BatchNorm2d (+ ReLU, + Dropout2d mask) of the auxiliary heads (reference nets/ShfitScaleFormer.py:329-368: Conv2d ->
 * BatchNorm2d -> ReLU -> Dropout2d(0.3)) on the channels-last matrix the convolution GEMM produces: x, y fp32 [M, C] with
 * M = samples * rows_per_sample.  training != 0: batch statistics (biased variance, eps inside the sqrt), running_mean /
 * running_var updated in place with `momentum` (unbiased variance), as torch.nn.BatchNorm2d; training == 0: the running
 * statistics.  mask: NULL or fp32 [samples, C] multipliers (0 or 1/(1-p): Dropout2d drops whole channels of a sample);
 * relu != 0 applies max(0, .) between the normalisation and the mask.  save_mean / save_rstd [C] are kept for backward.
 * workspace: dm_batchnorm_workspace_bytes(M, C), 8-byte aligned. */
int64_t dm_batchnorm_workspace_bytes(int32_t M, int32_t C);
int dm_batchnorm_fwd(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                     const float *mask, int32_t rows_per_sample, float *y, float *save_mean, float *save_rstd, int32_t M,
                     int32_t C, float eps, float momentum, int32_t training, int32_t relu, void *workspace, void *stream);
/* Gradient of the above (relu != 0: y > 0 decides the ReLU branch; pass the forward call's relu / training / mask): dx [M, C];
 * dgamma / dbeta [C] written, or added to when accumulate != 0. */
int dm_batchnorm_bwd(const float *dy, const float *x, const float *y, const float *gamma, const float *mask, int32_t rows_per_sample,
                     const float *save_mean, const float *save_rstd, float *dx, float *dgamma, float *dbeta, int32_t accumulate,
                     int32_t M, int32_t C, int32_t training, int32_t relu, void *workspace, void *stream);

/* ---- GRU cell (reference Nets.py:60-66: `nn.GRU(28, 80, num_layers=4, bidirectional=True)` of the MNIST sandbox net `RNN`) ----
 * PyTorch gate order r, z, n.  gi [B, 3H] with row stride gi_stride floats (a time slice of x W_ih^T + b_ih for all steps),
 * gh [B, 3H] = h W_hh^T + b_hh, h [B, H]:  r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r * gh_n),
 * h_new = (1 - z) * n + z * h.  saved [B, 4H] keeps r, z, n, gh_n for the backward call, which returns dgi, dgh [B, 3H] and
 * dh [B, H] (the direct path to the previous state; the caller adds the path through gh). */
int dm_gru_cell_fwd(const float *gi, int64_t gi_stride, const float *gh, const float *h, float *h_new, float *saved,
                    int32_t B, int32_t H, void *stream);
int dm_gru_cell_bwd(const float *dh_new, const float *saved, const float *h, float *dgi, float *dgh, float *dh, int32_t B,
                    int32_t H, void *stream);

/* ---- optional in-library kernel timing ------------------------------------------------------
 * While enabled, the GEMM and attention entry points bracket their main kernel with hipEvents on
 * the caller's stream.  dm_prof_collect waits for the recorded events, aggregates them per kernel
 * name (launch count, total milliseconds, total algorithmic FLOPs and bytes as computed from the
 * call's dimensions) and clears the log.  Used by bench.py for the roofline figure. */
typedef struct {
  char name[64];
  int64_t launches;
  double total_ms;
  double total_flops;
  double total_bytes;
} DmProfRow;
int dm_prof_enable(int32_t on);
int32_t dm_prof_collect(DmProfRow *rows, int32_t max_rows);

#ifdef __cplusplus
}
#endif
#endif /* DEEPMERGE_HIP_H */
