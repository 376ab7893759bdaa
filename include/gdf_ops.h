/* gdf_ops.h — kernel-level entry points of libgdf.so (diagnostics / unit tests / micro-benchmarks).
 * Same conventions as gdf.h: plain C, device pointers, asynchronous on `stream`, 0 = ok.
 * Each call is one launch of the kernel the plan executor uses for that op class.            */
#ifndef GDF_OPS_H
#define GDF_OPS_H
#include <stddef.h>
#include <stdint.h>

#include "gdf.h"    /* GDF_MAX_TIMESTEPS */
#ifdef __cplusplus
extern "C" {
#endif

/* out[M,N] = A[M,K](lda) * W[N,K]^T + bias (+ residual).  fp16 operands, fp32 accumulate.
 * flags: bit0 GEGLU (W rows / bias already interleaved [16 h | 16 gate] by gdf_op_relayout_geglu(group 16); out is
 *        [M,N/2]); bit1 narrow-N tile (BN=16; the GEGLU form has none: both bits together are an error);
 *        bits 8..19 force a tile variant (0 = auto; 16 / 128 / 160 / 256 / 320 = LDS-ring kernels of that tile, 932 / 825 / 826 =
 *        8-phase main loops: 256x320, 256x256 GEGLU, 256x256 conv; MMDiT forms: 128, 1256 / 2128 = 256x256 / 256x128 rings, 8256 =
 *        8-phase 256x256; any other number means the 128x128 tile, on MMDiT forms the automatic choice).  Operands larger than 2 GiB
 *        are rejected (GDF_ERR_UNSUPPORTED: 32-bit buffer offsets).  Replaces nn.Linear / 1x1 conv
 *        (/root/reference/feature/diffusers/models/attention_processor.py:241-267, attention.py:1238-1258). */
int gdf_op_gemm(const void* A, int lda, const void* W, const float* bias, const float* res32, const void* res16,
                int ldres, void* out16, int ldo16, float* out32, int ldo32, int M, int N, int K, int flags,
                void* stream);

/* 3x3 convolution, padding 1, NHWC fp16 x[B,H,W,ld>=Cin], weights in the layout gdf_op_relayout_conv3 produces
 * ([Cout][Cin/64][tap][64] fp16: channel-block-major, the nine taps innermost); stride 1|2;
 * ups=1 fuses a nearest x2 upsample of x in front of the conv.  rowvec: optional [B][Cout] fp32 added per sample.
 * Replaces nn.Conv2d in resnet.py:269,285, downsampling.py:115-118, upsampling.py:131-134,176-193.       */
int gdf_op_conv3x3(const void* x, int ld, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                   const float* rowvec, int stride, int ups, const float* res32, void* aux16, void* out16,
                   float* out32, int narrow /* bit0: BN=16; bits 8..: tile variant */, void* stream);

/* The complete GEMM / 3x3-conv launch: every field a plan builder sets (csrc/kernels.h GemmParams), one launch_gemm (or launch_gemm_splitk).
 *   A, lda       dense: fp16 (bf16 = 1: bf16) rows [M][lda]; conv3: NHWC x[B][H][W][lda >= Cin].  A column offset is part of the pointer.
 *   mode         0 dense (M, N, K), 1 conv3 (B, H, W, Cin, stride, ups, pad0; N = Cout; M and K are derived: M = B * OH * OW with
 *                OH = (IH - 1) / stride + 1, IH = ups ? 2 H : H, K = 9 * Cin).  pad0 = 1: zero padding right / bottom only.
 *   K            dense: the WEIGHT matrix's contraction size; a_lo > 0: A rows are split (hi | lo) pairs, lo a_lo elements after hi, and the
 *                launch contracts over 2 K (conv3 likewise per pixel).  The byte extents of A and W (out-of-range loads return 0) are
 *                derived as gdf_op_gemm_split / gdf_op_conv3x3_split derive them; operands of 2 GiB and more are rejected.
 *   W            [N][K] fp16 / bf16 (conv3: the gdf_op_relayout_conv3 layout; geglu: gdf_op_relayout_geglu(group 16) rows and bias).
 *   bias, rowvec fp32 [N] / [samples][ldrv]; rows_per_sample 0 = 1 (dense) or OH * OW (conv3); ldrv 0 = N.
 *   res32 | res16 (ldres), out16 (ldo16), out32 (ldo32), aux16 (ldaux): leading dimensions in elements, 0 = the output width (N, geglu: N / 2).
 *   bn           0 | 128, or 16 = the narrow-N tile; variant: a tile forced as in gdf_op_gemm's flags bits 8..19; one the form has no
 *                instantiation of (826 on a dense GEMM) is an error here and NULL from the query.
 *   splitk > 1   launch_gemm_splitk with the workspace splitk_ws (splitk * M * N floats).
 *   batch > 1    `batch` problems sharing A: problem b reads W + b * w_bstride and writes out16 + b * o_bstride (elements).
 *   dit          the MMDiT epilogue of gdf_op_gemm_dit: act, rv_mul, rv_seg_rows / rv_rps2, rv_tok (row vector per token: row % rows_per_sample),
 *                qkn_* (RMSNorm + rotary embedding on the q / k heads; position qkn_pos0 + row % qkn_rps, rows >= qkn_seg_rows > 0:
 *                qkn_pos1 + (row - qkn_seg_rows) % qkn_rps2; rope tables fp32 [position][128]), bf16 operands, out_f16 (saturating fp16 store).
 *   acc_scale, out16_scale   v = acc * acc_scale + bias ...; out16 = e16(v * out16_scale); 0 means 1.
 *   o16_lo > 0   out16 is written as a split (hi, lo) pair, lo o16_lo elements after hi in the same row.
 *   cus > 0      tile choice, persistent grid and super-block order as on a stream restricted to `cus` CUs.
 *   conv3 with Cin <= 8   the conv_in form (what gdf_op_conv_in prepares in its scratch): A is the image as NHWC pixels of 8 packed fp16
 *                channels (channels from Cin up zero; lda is not read), W is [N][16 taps][8 channels] (taps from 9 up and channels from Cin up
 *                zero); stride 1, no ups / pad0 / a_lo.  Every epilogue field applies, o16_lo included (the conv_in of a "precise" plan).
 *   mx           gdf_op_gemm_kernel only: the fp8 form of gdf_op_gemm_mx (K in bytes, a multiple of 128); gdf_op_gemm_ex refuses it. */
typedef struct gdf_gemm_args {
  const void* A; int lda;
  const void* W;
  int mode;
  int M, N, K;
  int B, H, Wd, Cin, stride, ups, pad0;
  const float* bias;
  const float* rowvec; int rows_per_sample, ldrv;
  const float* res32; const void* res16; int ldres;
  void* out16; int ldo16;
  float* out32; int ldo32;
  void* aux16; int ldaux;
  int geglu, bn, variant, no_superblock;
  int splitk; float* splitk_ws;
  int batch; long w_bstride, o_bstride;
  int dit, act, rv_mul, rv_seg_rows, rv_rps2, rv_tok;
  int qkn_nq; const float* qkn_wq; const float* qkn_wk; float qkn_eps; const float* rope_cos; const float* rope_sin;
  int qkn_pos0, qkn_rps, qkn_seg_rows, qkn_pos1, qkn_rps2;
  int bf16, out_f16;
  float acc_scale, out16_scale;
  int a_lo, o16_lo;
  int cus;
  int mx;
} gdf_gemm_args;
int gdf_op_gemm_ex(const gdf_gemm_args* args, void* stream);
/* Symbol of the GEMM kernel gdf_op_gemm_ex launches for these arguments, as a profiler prints it without namespace and signature
 * ("gemm_kernel<1, 256, 320, 9, false>": mode, tile rows, tile columns, stages (8 / 9: the 8-phase main loops), GEGLU;
 * "gemm_dit_kernel<256, 256, 8, true, false>": tile, stages, bf16, QKN).  With splitk > 1: the kernel of the partial-sum launch.
 * Host arithmetic only: no device is touched and no pointer is followed (only whether res32 / res16 / rowvec / aux16 / out32 are set
 * matters).  NULL for arguments the launch rejects and for an empty problem.  The string lives as long as the library. */
const char* gdf_op_gemm_kernel(const gdf_gemm_args* args);

/* SPLIT-OPERAND forms (the opt-in "precise" plans, gdf.h gdf_plan_opts.reserved[1]): an activation is a pair of fp16 numbers
 * hi = fp16(v), lo = fp16(v - hi) stored in ONE row, lo `a_lo` (input) / `o16_lo` / `y_lo` / `o_lo` (output) elements after hi, and a
 * contraction runs over [hi | lo] against the weight matrix read twice: out = (hi + lo) W^T to fp32 accuracy.  a_lo = 0 / *_lo = 0:
 * the plain form.  Kw / Cin are the WEIGHT matrix's contraction sizes.  They replace the same reference call sites as their
 * plain counterparts; the reference itself has no such mode (it rounds more: fp16 activations AND an fp16 residual stream). */
int gdf_op_gemm_split(const void* A, int lda, int a_lo, const void* W, const float* bias, const float* res32, int ldres, void* out16,
                      int ldo16, int o16_lo, float* out32, int ldo32, int M, int N, int Kw, int flags /* bit0 GEGLU */, void* stream);
int gdf_op_conv3x3_split(const void* x, int ld, int a_lo, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                         int stride, int ups, const float* res32, void* out16, int ldo16, int o16_lo, float* out32, void* stream);
int gdf_op_layernorm_split(const float* x32, int ld, int R, int C, float eps, const float* gamma, const float* beta, void* y, int ldy,
                           int y_lo, void* stream);
/* x: fp32 (x32, ld) or a split fp16 pair (x16, ld, x_lo) */
int gdf_op_groupnorm_split(const void* x16, int x_lo, const float* x32, int ld, int B, int HW, int C, int G, float eps, const float* gamma,
                           const float* beta, int silu, void* y, int ldy, int y_lo, void* scratch, void* stream);
int gdf_op_attention_split(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int o_lo, int B,
                           int heads, int Sq, int Sk, int D, void* map, void* stream);

/* q, k and v as split pairs (hi, lo = fp16(x - hi), lo at +qkv_lo elements in the same row: what a GEMM with o16_lo writes): the softmax sees
 * q k^T contracted over both halves, O accumulates P (v_hi + v_lo) — the full-split UNet plans (attention_processor.py:3311-3313 in fp32 terms).
 * Head dims 40 <= D <= 80 (40 / 64 / 72 / 80); others read the hi halves only. */
int gdf_op_attention_pair(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int qkv_lo, void* o, int ldo, int o_lo, int B,
                          int heads, int Sq, int Sk, int D, void* stream);

/* Deterministic split-K form of gdf_op_conv3x3 (few output tiles, long K — the 8x8-level convs of SD1.5): the K range is cut
 * into `splitk` contiguous parts (0 = the plan builder's heuristic, gdf_op_splitk_factor), every part writes raw fp32 partial
 * sums to its own slab of `ws` (splitk * M * Cout floats, M = B * OH * OW), a second kernel adds the slabs in a fixed order and
 * applies the same epilogue as gdf_op_conv3x3.  Same result as the unsplit conv up to fp32 summation order. */
int gdf_op_conv3x3_splitk(const void* x, int ld, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                          const float* rowvec, int stride, int ups, const float* res32, void* aux16, void* out16,
                          float* out32, int splitk, float* ws, void* stream);
int gdf_op_splitk_factor(int M, int N, int K, int conv);

/* conv_in: x NCHW fp16 [B,Cin<=8,H,W] -> NHWC [B,H,W,Cout]; weights in diffusers OIHW fp16 layout.
 * scratch: B*H*W*16 + Cout*256 bytes.                                                                  */
int gdf_op_conv_in(const void* x_nchw, int B, int Cin, int H, int W, const void* w_oihw, const float* bias, int Cout,
                   void* out16, void* scratch, void* stream);

/* softmax(q k^T * D^-0.5) v per head; rows are tokens, head h at columns [h*D, h*D+D).
 * map != NULL additionally writes the probabilities (B, heads, Sq, Sk) fp16 ('-map' hooks).
 * Replaces F.scaled_dot_product_attention (attention_processor.py:3311-3313) /
 * get_attention_scores+bmm (attention_processor.py:640-685, components/attention.py:232-246).          */
int gdf_op_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                     int B, int heads, int Sq, int Sk, int D, void* map, void* stream);

/* The complete attention launch: every field a plan can set (csrc/kernels.h AttnParams), one kernel launch.
 *   q / k / v / o: rows are tokens, head h at columns [h*D, h*D+D), leading dimensions in elements (ldq / ldk / ldv % 8 == 0, ldo % 4 == 0).
 *   kv_bstride  rows between consecutive samples' K / V (Sk normally; 0 = all samples share one K / V set).
 *   scale       softmax scale; 0 = D^-0.5.
 *   map         optional probabilities (B, heads, Sq, Sk) fp16; with seg_T > 0 the `self-map` (B, heads, Sq - seg_T, Sk - seg_T).
 *   map2        seg_T > 0 only: the `cross-map` (B, heads, Sq - seg_T, seg_T) (image queries x text keys).  Maps need seg_T % 8 == 0.
 *   kv_len      optional device int[B]: keys [max(1, min(kv_len[b], Sk)), Sk) of sample b are masked out (probability 0).
 *   seg_T       > 0: MMDiT joint sequence, rows region-major [B x seg_T text][B x (Sq - seg_T) image], Sq == Sk.
 *   bf16        D = 128 only: q, k, v, o are bf16; maps stay fp16.
 *   o_lo        > 0: o is written as a split (hi, lo) pair, lo at +o_lo elements in the same row; o_pair_bf16: the pair is bf16 hi + bf16 lo
 *               (fp16 q / k / v only).
 *   q_lo, kv_lo both > 0 (fp16, 40 <= D <= 80): q, k, v are split pairs, lo at +q_lo / +kv_lo elements in the same row.
 *   o_scale     != 0: o is stored multiplied by this power of two. */
typedef struct gdf_attn_args {
  const void* q; int ldq;
  const void* k; int ldk;
  const void* v; int ldv;
  void* o; int ldo;
  int B, heads, Sq, Sk, D;
  int kv_bstride;
  float scale;
  void* map;
  void* map2;
  const int* kv_len;
  int seg_T;
  int bf16;
  int o_lo;
  int o_pair_bf16;
  int q_lo, kv_lo;
  float o_scale;
} gdf_attn_args;
int gdf_op_attention_ex(const gdf_attn_args* args, void* stream);
/* Symbol of the kernel gdf_op_attention_ex launches for these arguments, as a profiler prints it without namespace and signature
 * ("attn_kernel<64, 2, 4, false, 2, false, false>", "attn_map_kernel<40, true, 3, true, false>").  Host arithmetic only: no device
 * is touched and no pointer is followed (only whether map / map2 / kv_len are set matters).  NULL for arguments the launch rejects.
 * The string lives as long as the library. */
const char* gdf_op_attention_kernel(const gdf_attn_args* args);

/* GroupNorm(G groups, eps) [+SiLU] over NHWC x (fp16, ld) or x32 (fp32, ld); y contiguous fp16 [B*HW][C].
 * scratch: gdf_op_groupnorm_scratch_bytes(B,HW,C).                                                      */
size_t gdf_op_groupnorm_scratch_bytes(int B, int HW, int C);
int gdf_op_groupnorm(const void* x16, const float* x32, int ld, int B, int HW, int C, int G, float eps,
                     const float* gamma, const float* beta, int silu, void* y, void* scratch, void* stream);

/* The GroupNorm producers one at a time.  The affine table ab[b][c] = (rstd * gamma[c], beta[c] - mean * rstd * gamma[c]) (fp32 pairs) comes
 * from the single-launch kernel (which keeps it in LDS), from gdf_op_gn_stats, or from a conv epilogue's per-slab channel sums
 * (gdf_op_conv3x3_gn) through gdf_op_gn_finalize; gdf_op_gn_apply is y = act(x * a + b).
 *   gdf_op_gn_path        host arithmetic only: *fused_sc = channels per workgroup of the single-launch kernel (0: gdf_op_groupnorm takes the
 *                         statistics + apply path), *slab_rows / *nslab = pixel rows per slab and slabs per sample of gdf_op_gn_stats.
 *   gdf_op_gn_stats       partial: scratch of B * nslab * C * 2 floats; x fp16 (x16, ld), a split pair (x_lo > 0) or fp32 (x32, ld).
 *   gdf_op_gn_apply       y fp16 rows of ldy elements (0 = C); y_lo > 0: a split (hi, lo) pair, lo at column offset y_lo.
 *   gdf_op_gn_finalize    partial: [B][nslab][C][2] = (sum x, sum x^2) per slab and channel; HW = pixels per sample the sums cover;
 *                         fold: scratch of gdf_op_gn_fold_floats(B, nslab, C) floats, or NULL (0 floats: no pre-reduction is used). */
int gdf_op_gn_path(int B, int HW, int C, int G, int* fused_sc, int* slab_rows, int* nslab);
int gdf_op_gn_stats(const void* x16, int x_lo, const float* x32, int ld, int B, int HW, int C, int G, float eps, const float* gamma,
                    const float* beta, float* partial, float* ab, void* stream);
int gdf_op_gn_apply(const void* x16, int x_lo, const float* x32, int ld, int B, int HW, int C, const float* ab, int silu, void* y,
                    int ldy, int y_lo, void* stream);
int gdf_op_gn_finalize(const float* partial, int nslab, int B, int HW, int C, int G, float eps, const float* gamma, const float* beta,
                       float* ab, float* fold, void* stream);
size_t gdf_op_gn_fold_floats(int B, int nslab, int C);

/* gdf_op_conv3x3 / gdf_op_conv_in whose epilogue also writes the GroupNorm partial sums of the stored image: out16 = fp16(v * out16_scale)
 * (0 means 1) and gn_partial[row / slab_rows][c] = (sum, sum of squares) of v * out16_scale over that slab's rows, M / slab_rows slabs of
 * Cout pairs.  An error (nothing is launched) where the tile has no such epilogue or M is not a whole number of slabs.
 * gdf_op_conv3x3_gn_info: host arithmetic only; the kernel symbol ("gemm_gn_kernel<1, 256, 320, 9>": mode, tile rows, tile columns, stages)
 * and *slab_rows for these sizes and tile bits, NULL and 0 where the launch is refused.  Cin <= 8 asks about the conv_in form. */
int gdf_op_conv3x3_gn(const void* x, int ld, int B, int H, int W, int Cin, const void* Wt, int Cout, const float* bias,
                      const float* rowvec, int stride, int ups, const float* res32, void* aux16, void* out16,
                      float* out32, int narrow, float out16_scale, float* gn_partial, void* stream);
int gdf_op_conv_in_gn(const void* x_nchw, int B, int Cin, int H, int W, const void* w_oihw, const float* bias, int Cout,
                      void* out16, void* scratch, float out16_scale, float* gn_partial, void* stream);
const char* gdf_op_conv3x3_gn_info(int B, int H, int W, int Cin, int Cout, int stride, int ups, int flags, int* slab_rows);

/* LayerNorm over the last dim. */
int gdf_op_layernorm(const void* x16, const float* x32, int ld, int R, int C, float eps, const float* gamma,
                     const float* beta, void* y, void* stream);

/* strided fp16/fp32 -> fp16 2-D copy (the hook-store kernel). */
int gdf_op_copy2d(const void* s16, const float* s32, int lds, void* dst, int ldd, int R, int C, void* stream);

/* The same kernel with every argument of its launcher: src_bf16: s16 holds bf16; sat: the fp16 store saturates at +-65504 instead of
 * overflowing to +-inf (NaN stays NaN); s_lo > 0: the 16-bit source is a split (hi, lo) pair, lo s_lo elements after hi in the row, and
 * dst = fp16(hi + lo); dst = fp16(scale * src).  Any of these selects the MMDiT hook form copy2d_kernel<true>.  C, lds and ldd all
 * multiples of 8: 16-byte lanes; otherwise one element per lane. */
int gdf_op_copy2d_ex(const void* s16, const float* s32, int lds, void* dst, int ldd, int R, int C, int src_bf16, int sat, int s_lo, float scale,
                     void* stream);

/* ---- embedding, packing, patch-layout and VAE head / tail kernels (csrc/norm.hip, csrc/dit.hip), one launch each ---- */

/* get_timestep_embedding(flip_sin_to_cos = True, downscale_freq_shift = 0): t fp32 [B][n_per_row] ->
 * out[b][col_off + i * dim + j] = j < dim / 2 ? cos(a) : sin(a), a = t[b][i] * tscale * exp(-ln(10000) * (j mod dim / 2) / (dim / 2)),
 * fp32 rows of ldo; round_f16: every value rounded to fp16 first (the reference's fp16 embedding). */
int gdf_op_sinusoid(const float* t, int B, int n_per_row, int dim, float* out, int ldo, int col_off, int round_f16, float tscale, void* stream);
/* out[b][col_off + j] = x[b][j]: 16-bit rows [B][n] (fp16, src_bf16 = 1: bf16) widened into fp32 rows of ldo. */
int gdf_op_widen(const void* x, int src_bf16, int B, int n, float* out, int ldo, int col_off, void* stream);
/* out[i] = x[i] / (1 + exp(-x[i])), fp32. */
int gdf_op_silu_vec(const float* x, float* out, long n, void* stream);
/* out[b][i] = table[i] + vec[b][i mod period], fp32; vec rows of ldvec, out rows of ldo (ada_norm_single's scale_shift_table). */
int gdf_op_add_table(const float* table, const float* vec, int ldvec, int period, int B, long n, float* out, long ldo, void* stream);
/* latents NCHW fp16 (B, Cin <= 8, H, W) -> NHWC pixels of 8 fp16 channels (channels from Cin up zero: the conv_in operand) and, if
 * hook_nhwc != NULL, the plain NHWC copy (B, H, W, Cin). */
int gdf_op_pack_latents(const void* x_nchw, int B, int Cin, int H, int W, void* nhwc8, void* hook_nhwc, void* stream);
/* latents NCHW fp16 (B, Cin, H, W) -> patch rows [B * (H / p) * (W / p)][kpad] fp16, column (c * p + py) * p + px (the Conv2d weight
 * order), columns from Cin * p * p up zero.  H % p == 0, W % p == 0, Cin * p * p <= kpad. */
int gdf_op_patchify(const void* x_nchw, int B, int Cin, int H, int W, int p, int kpad, void* out, void* stream);
/* token rows [B * gh * gw][p * p * Cout] fp16, column (py * p + px) * Cout + c -> NCHW fp16 (B, Cout, gh * p, gw * p)
 * (the `nhwpqc -> nchpwq` einsum of transformer_2d.py:563-570). */
int gdf_op_unpatchify(const void* x, int B, int Cout, int gh, int gw, int p, void* out_nchw, void* stream);
/* VAE encoder tail: moments = quant_conv(h) (1x1: wq fp16 [2L][2L], bq fp32 [2L] or NULL = 0; wq == NULL: identity) of h fp32 [B * HW][2L],
 * (mean | logvar) split, z = mean + exp(0.5 * clamp(logvar, -30, 20)) * eps (eps == NULL: the mode), lat = scaling * z,
 * out = in_scale * (noise_a * lat + noise_b * noise) (noise == NULL: in_scale * lat) -> NCHW fp16 (B, L, HW); eps, noise NCHW fp16.  L <= 8. */
int gdf_op_vae_finish(const float* h, int B, int HW, int L, const void* wq, const float* bq, const void* eps, const void* noise, float scaling,
                      float noise_a, float noise_b, float in_scale, void* out, void* stream);
/* The same tail for n_t timesteps of the same B images, 1 <= n_t <= GDF_MAX_TIMESTEPS: the moments are read and quant_conv applied once per
 * (image, pixel); eps, noise and out are NCHW fp16 (n_t * B, L, HW), TIMESTEP-MAJOR — row k * B + b is image b at timestep k and uses
 * noise_a[k], noise_b[k], in_scale[k].  The three arrays are HOST pointers of n_t floats (they travel in the kernel arguments: no device
 * table, no copy).  Per element the result has the bits gdf_op_vae_finish gives for the same operands.  L <= 8. */
int gdf_op_vae_finish_multi(const float* h, int B, int HW, int L, const void* wq, const float* bq, const void* eps, const void* noise,
                            float scaling, int n_t, const float* noise_a, const float* noise_b, const float* in_scale, void* out, void* stream);
/* The Flux latent-preparation tail, 1 <= L <= 16, H and W even: the same moments (h fp32 [B * H * W][2L]; quant_conv as above, NULL for the Flux
 * VAE), out = noise_a * scaling * ((mean - shift) + std * eps) + noise_b * noise — gdf_op_vae_finish's value on (mean - shift) with in_scale = 1,
 * so at shift = 0 the same bits — computed in fp32, rounded once to fp16 or bf16 (out_bf16) and written as 2x2-packed token rows
 * (B, (H/2) * (W/2), 4L): element [b][gy * (W/2) + gx][c * 4 + dy * 2 + dx] is latent (b, c, 2gy + dy, 2gx + dx), the layout of
 * FluxImg2ImgPipeline._pack_latents.  eps, noise NCHW fp16 (B, L, H, W) or NULL.  L > 16, odd H or W, a null out: an error, nothing written. */
int gdf_op_vae_finish_packed(const float* h, int B, int H, int W, int L, const void* wq, const float* bq, const void* eps, const void* noise,
                             float scaling, float shift, float noise_a, float noise_b, int out_bf16, void* out, void* stream);
/* VAE decoder head: z = (c_sample * latents + c_eps * noise_pred) * inv_scaling (noise_pred == NULL: no second term), y = post_quant_conv(z)
 * (1x1: wq fp16 [L][L], bq fp32 [L] or NULL = 0; wq == NULL: identity) -> NHWC pixels of 8 fp16 channels, channels from L up zero.
 * latents, noise_pred NCHW fp16 (B, L, HW).  L <= 8. */
int gdf_op_vae_dec_prepare(const void* latents, const void* noise_pred, int B, int HW, int L, float c_sample, float c_eps, float inv_scaling,
                           const void* wq, const float* bq, void* nhwc8, void* stream);

/* ---- weight re-layouts of model load time; src_dtype: 0 fp16, 1 fp32, 2 bf16 ---- */
/* dst[r][0..kdst) = fp16(src[r][0..ksrc)) zero padded; src fp16 or fp32 (src_f32). */
int gdf_op_relayout_rows_padk(const void* src, int src_f32, void* dst, int R, int ksrc, int kdst, void* stream);
/* OIHW weights src[O][I][T] (T = kh * kw) -> fp16 dst[O][tpad][ipad] (cblk = 0: dst[o][t][i] = src[o][i][t]) or, cblk > 0,
 * dst[O][ipad / cblk][tpad][cblk] (dst[o][i / cblk][t][i % cblk]); i >= I and t >= T are zero.  ipad % cblk == 0. */
int gdf_op_relayout_conv(const void* src, int src_dtype, void* dst, int O, int I, int T, int ipad, int tpad, int cblk, void* stream);
/* dst[map(r)][k] = e16(src[r][k]), r < R, rows of K; geglu = 0: map(r) = r + row_off; geglu = g: the [g h | g gate] interleave of the
 * [h rows | gate rows] matrix (R / 2 a multiple of g; row_off is not used).  dst fp16, or bf16 (dst_bf16), rounded to nearest even. */
int gdf_op_relayout_rows(const void* src, int src_dtype, void* dst, int R, int K, int row_off, int geglu, int dst_bf16, void* stream);
/* the same row mapping for a vector, to fp32: dst[map(r)] = src[r]. */
int gdf_op_relayout_vec(const void* src, int src_dtype, float* dst, int R, int row_off, int geglu, void* stream);

/* weight re-layout helpers used by the tests: OIHW -> OHWI, GEGLU row interleave. */
int gdf_op_relayout_conv3(const void* w_oihw_f16, void* dst, int O, int I, void* stream);
int gdf_op_relayout_geglu(const void* w_f16, const float* bias, void* w_dst, float* bias_dst, int R, int K, int group /*16*/, void* stream);

/* out[m][n] = (accumulate ? out : 0) + bias[n] + sum_k act(x[m][k]) W[n][k]; x fp32 [M][ldx] (M small), W fp16 [N][K], out fp32.
 * The time / text / adaLN-modulation embedding linears (unet_2d_condition.py:1142-1162, resnet.py:343-346; MMDiT adaLN
 * `linear(silu(temb))`, stacked over all blocks: N = 1.06 M columns -> LDS-staged wide kernel).                          */
int gdf_op_small_linear(const float* x, int ldx, int M, int K, const void* W, const float* bias, int N, int silu_in,
                        int accumulate, float* out, int ldo, void* stream);

/* The same launch with the weights' storage type: w_bf16 = 1: W holds bf16 (the MMDiT's bf16 models). */
int gdf_op_small_linear_ex(const float* x, int ldx, int M, int K, const void* W, int w_bf16, const float* bias, int N, int silu_in,
                           int accumulate, float* out, int ldo, void* stream);

/* in-place row softmax of fp16 scores: x[r][0..n) = softmax(scale * x[r][0..n)) with fp32 math (VAE mid-block attention,
 * attention_processor.py:3311-3313 run as explicit GEMMs; n <= 16384, n % 8 == 0). */
int gdf_op_softmax_rows(void* x, int ld, int R, int n, float scale, void* stream);

/* PatchEmbed positional table (PixArt): out fp32 [gh*gw][C] = get_2d_sincos_pos_embed(C, (gh, gw), base_size, interpolation_scale). */
int gdf_op_sincos_pos_embed(float* out, int C, int gh, int gw, int base_size, float interpolation_scale, void* stream);

/* ---- output-stage post-processing (csrc/post.hip) ---- */

/* `--aggregate_output` (extract_feature.py:113-125): nearest-resize one layer — logical (B,C,H,W), element strides
 * sb/sc/sy/sx, fp16 (src_f32 = 0) or fp32 — to S x S (PyTorch `nearest`: floor(dst * in / out)) and store it as channels
 * [coff, coff + C) of out (B, Ctot, S, S) fp16 contiguous; one call per layer performs F.interpolate + torch.cat(dim=1). */
int gdf_op_resize_concat(const void* src, int src_f32, long sb, long sc, long sy, long sx, int B, int C, int H, int W, void* out,
                         int Ctot, int coff, int S, void* stream);
/* The evaluators' form of the same stage (correspondence/aggregation_network.py:62-66, scarce_segmentation/task-pixel.py:50-55):
 * torch.cat([F.interpolate(v, (OH, OW), mode='bilinear') for v in feats], 1) — ONE launch of aggregate_kernel over n <= 16 sources.
 *   srcs   source l is a logical (B, C, H, W) tensor, fp16 (f32 = 0) or fp32, with element strides sb/sc/sy/sx (hooks: channels-last, sc = 1;
 *          `attn`: NCHW), read only; it lands in channels [coff, coff + C) of out.  Callers with more sources make several calls.
 *   out    (B, Ctot, OH, OW) contiguous, fp16 (out_f32 = 0) or fp32; channels no source names are not written
 *   mode   1 bilinear: align_corners = False, no antialias, as ATen's upsample_bilinear2d: in fp32, scale = (float)in / out,
 *          src = max(0, scale * (dst + 0.5f) - 0.5f), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1; the four taps are
 *          combined in fp32 and rounded once.  Where H == OH and W == OW the result is the source value cast to the output type.
 *          0 nearest: the bits of gdf_op_resize_concat, one launch of its kernel per source; fp16 output and OH == OW only.
 * Stream-ordered, no workspace, nothing read back.  n < 1 or > 16, a null pointer, C, H, W, OH or OW below 1, B < 0, coff < 0 or
 * coff + C > Ctot, an unknown mode, or nearest with out_f32 or OH != OW: GDF_ERR_ARG before any launch.  B == 0 is a successful no-op. */
typedef struct gdf_agg_src { const void* ptr; int f32; long sb, sc, sy, sx; int C, H, W, coff; } gdf_agg_src;
int gdf_op_aggregate(const gdf_agg_src* srcs, int n, int B, void* out, int out_f32, int Ctot, int OH, int OW,
                     int mode /* 0 nearest, 1 bilinear */, void* stream);
/* The evaluators' second step on two aggregated maps (correspondence/correspondence/correspondence_utils.py:113-138,
 * find_nn_source_correspondences, called per image pair from correspondence/task-corres.py:110): both maps F.interpolate'd to the load size
 * (LH, LW) (bilinear), the N source points gathered from the first, both sides L2-normalised, sims = q @ k^T, argmax over the LH * LW target
 * pixels — computed WITHOUT either load-size map (csrc/corres.hip): one pass over the coarse target yields <q_n, T> and five
 * neighbour products per coarse pixel; a pass over the fine grid blends them, divides by the Gram-form norm and reduces.
 *   f1, f2     logical (B, C, H, W) tensors, fp16 (f32 = 0) or fp32 independently, with element strides sb/sc/sy/sx, read only; the two C must
 *              agree, the grids need not; `coff` is ignored.  A target with sx == 1 (NCHW, what gdf_op_aggregate writes) is read with lanes along
 *              x; one with sc == 1, C a multiple of 8 (fp32: 4) and 16-byte aligned pixels (a channels-last hook) with 16-byte loads along C;
 *              any other strides are correct, not fast.
 *   points     device, (B, N, 2) fp32, (y, x) in load-size coordinates.  Source index: y = round_half_even(clip(y, 0, LH - 1)), x likewise with
 *              LW (points_to_idxs, np.round); the query is the bilinear sample of f1 there — its four taps — normalised in fp32.
 *   upsampling ATen's upsample_bilinear2d, align_corners = False, with the fp32 coordinate arithmetic of gdf_op_aggregate mode 1 above; where the
 *              second tap clamps onto the first (i1 == i0) its weight is taken as 0.
 *   score      s[n, p] = <q_n, v_p> / ||v_p|| in fp32 throughout.  out_yx (B, N, 2) int64 = (p* / LW, p* % LW) of the LOWEST flat index p* of
 *              maximal computed score (argmax's rule), out_score (B, N) fp32 the score there.
 *   zero norms a target pixel whose computed norm is not positive never wins; a query of norm 0 (or one no pixel answers) returns index 0 and a
 *              NaN score — the reference propagates NaN here.
 *   workspace  gdf_op_nn_match_workspace(B, N, C, h2, w2) bytes (h2, w2: the grid of f2), 16-byte aligned, caller-owned, contents undefined
 *              before and after.  Any N: queries are processed 24 at a time.
 * Stream-ordered, nothing read back, no allocation; the same inputs give the same bits on any stream.  A null pointer, C, H, W, LH, LW or N
 * below 1, differing C, B < 0, a misaligned or too small workspace: GDF_ERR_ARG before any launch.  B > 65535, LH * LW >= 2^30 or
 * B * h2 * w2 >= 2^31: GDF_ERR_UNSUPPORTED.  B == 0 is a successful no-op. */
size_t gdf_op_nn_match_workspace(int B, int N, int C, int h2, int w2);
int gdf_op_nn_match(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, const float* points /* device, (B, N, 2) */, int N, int LH, int LW,
                    long long* out_yx /* (B, N, 2) */, float* out_score /* (B, N) */, void* workspace, size_t workspace_bytes, void* stream);
/* Dense matching of two descriptor maps (correspondence/correspondence/correspondence_utils.py:73-111, batch_cosine_sim + find_nn_correspondences,
 * and :264-274, the similarity matrix and the two torch.max of find_best_buddies_correspondences): both maps flattened and L2-normalised,
 * sims = f1^ @ f2^T (B, P1, P2), argmax / max along both axes — computed WITHOUT the matrix (csrc/densematch.hip): one tiled MFMA
 * pass with fp32 accumulation whose epilogue reduces each 256 x 256 tile to per-row and per-column (score, index) partials.
 *   f1, f2     logical (B, C, H, W) tensors, fp16 (f32 = 0) or fp32 independently, with element strides sb/sc/sy/sx (NCHW, channels-last or any
 *              other), read only and once; the two C must agree, the grids need not (P1 = H1 W1, P2 = H2 W2, pixel p = y W + x); `coff` is ignored.
 *   operands   an fp16 map enters the product as it is, its 1 / ||v|| (fp32) is applied in the epilogue: the fp16 x fp16 products are exact in the
 *              fp32 accumulator.  An fp32 map is normalised in fp32 and enters as a scaled fp16 (hi, lo) pair: two or three MFMA passes per K
 *              step, lo x lo dropped.  The order of summation over C is the same for every pixel pair.
 *   score      s[p1, p2] = (dot * r1[p1]) * r2[p2], evaluated once in fp32; both directions reduce these same bits, so nn21[nn12[p]] == p is a
 *              consistent mutual-nearest-neighbour test.  Error bound on the cosine: (2 C + 16) 2^-24 for fp16 maps (tests/dense_match_ref.py
 *              derives it, and the term of an fp32 map).
 *   outputs    nn12 (B, P1) int32: the LOWEST p2 of maximal computed score (argmax's rule), sim12 (B, P1) fp32: the score there; nn21 (B, P2),
 *              sim21 (B, P2) likewise for every pixel of f2 over the pixels of f1.  A pair (nn12, sim12) or (nn21, sim21) may be null: that
 *              direction is not reduced and nothing of it is written.  Half a pair, or both pairs null: GDF_ERR_ARG.
 *   zero norms a pixel whose computed norm is not positive and finite never wins; its own row (column), or one that no pixel answers, returns
 *              index 0 and a NaN score, as gdf_op_nn_match does — the reference propagates NaN here.
 *   workspace  gdf_op_dense_match_workspace(B, C, P1, P2, f32_1, f32_2) bytes, 16-byte aligned, caller-owned, contents undefined before and
 *              after: the fp16 operand panels (2 bytes per element of an fp16 map, 4 of an fp32 map, pixels padded to 256 and C to 64), the
 *              reciprocal norms and the tile partials.
 * Stream-ordered, no allocation, no atomics, nothing read back; the same inputs give the same bits on any stream, on repeated calls and at any
 * batch position.  A null map, C, H or W below 1, differing C, B < 0, a misaligned or too small workspace: GDF_ERR_ARG before any launch.
 * B > 65535, a map of more than 2^30 pixels, or 2^31 tiles or more: GDF_ERR_UNSUPPORTED.  B == 0 is a successful no-op. */
size_t gdf_op_dense_match_workspace(int B, int C, int P1, int P2, int f32_1, int f32_2);
int gdf_op_dense_match(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, int* nn12 /* (B, P1) */, float* sim12 /* (B, P1) */,
                       int* nn21 /* (B, P2) */, float* sim21 /* (B, P2) */, void* workspace, size_t workspace_bytes, void* stream);
/* The correspondence evaluator's loss on two hyperfeature maps (correspondence/task-corres.py:70-80, compute_clip_loss, called per image pair from
 * validate() :103 and per step from train() :159) and its gradient with respect to both maps — computed WITHOUT either P x P similarity matrix
 * (csrc/cliploss.hip).  With a^_p = f1[:, p] / ||f1[:, p]|| and b^_p likewise for f2 (pixel p = y W + x):
 *     direction 1   z[n, p] = scale <a^_src[n], b^_p>,   term1[n] = logsumexp_p z[n, p] - z[n, tgt[n]]
 *     direction 2   the roles swapped: queries b^_tgt[n], keys a^_p, labels src[n]
 *     loss = (mean_n term1 + mean_n term2) / 2
 *   f1, f2     logical (B, C, H, W) tensors, fp16 (f32 = 0) or fp32 independently, with element strides sb/sc/sy/sx, read only; the two C must
 *              agree, the grids need not; `coff` is ignored.  A map with sx == 1 (NCHW, what gdf_agghead_forward and gdf_op_aggregate write) is read
 *              with lanes along the pixels; one with sc == 1, C a multiple of 8 (fp32: 4) and 16-byte aligned pixels with 16-byte loads along C;
 *              any other strides are correct, not fast.
 *   src_idx, tgt_idx   device, (B, N) int64: flat pixel indices into f1 (P1 = H1 W1 pixels) and f2 (P2).  Duplicates are allowed.
 *   scale      exp(logit_scale), 1 / 0.07 in the reference; positive and finite.  The log-sum-exp subtracts the exact maximum.
 *   loss       (B) fp32, one value per pair.  terms, if not null: (B, 2, N) fp32, the 2 N cross-entropy terms before the means, direction 1 first.
 *   backward   grad_loss: device, (B) fp32, the upstream gradient.  grad_f1 (B, C, H1, W1) and grad_f2 (B, C, H2, W2): fp32 contiguous, every
 *              element written; either may be null and the other's bits do not depend on that.  With G[n, p] = grad_loss scale / (2 N)
 *              (softmax_p(z[n, .])[p] - [p == label_n]) every key pixel receives (sum_n G[n, p] q^_n - k^_p sum_n G[n, p] cos[n, p]) / ||k_p|| and
 *              every query pixel (sum_p G[n, p] k^_p - q^_n sum_p G[n, p] cos[n, p]) / ||q_n|| on top, duplicates accumulating in n order.
 *   workspace  gdf_op_clip_loss_workspace(B, N, C, P1, P2) bytes, 16-byte aligned, caller-owned.  After the forward call it holds the state of the
 *              backward (cos of both directions, the inverse norms, the log-sum-exps, a validity flag per pair) in an opaque layout, and the space
 *              for the backward's partial sums; the backward requires the same arguments and that workspace untouched, and may be called
 *              repeatedly.  Any N: queries are processed 24 at a time.
 *   invalid pairs   an index outside its map, or a pixel of zero or non-finite norm anywhere in either map of a pair (the reference's 0 / 0):
 *              that pair's loss, terms and gradients are all NaN, nothing outside the maps is read or written, other pairs are unaffected.
 * fp32 throughout, no atomics, every reduction in a fixed order: the same inputs give the same bits on any stream and at any batch position.
 * Stream-ordered, nothing read back, no allocation.  A null required pointer, C, H, W or N below 1, differing C, B < 0, a scale that is not
 * positive and finite, a misaligned or too small workspace: GDF_ERR_ARG before any launch.  B > 65535 or H * W >= 2^30: GDF_ERR_UNSUPPORTED.
 * B == 0 is a successful no-op. */
size_t gdf_op_clip_loss_workspace(int B, int N, int C, int P1, int P2);
int gdf_op_clip_loss(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, const long long* src_idx, const long long* tgt_idx /* device, (B, N) */,
                     int N, float scale, float* loss /* (B) */, float* terms /* (B, 2, N) or NULL */, void* workspace, size_t workspace_bytes,
                     void* stream);
int gdf_op_clip_loss_backward(const gdf_agg_src* f1, const gdf_agg_src* f2, int B, const long long* src_idx, const long long* tgt_idx, int N,
                              float scale, const float* grad_loss /* device, (B) */, float* grad_f1 /* (B, C, H1, W1) fp32 contiguous, or NULL */,
                              float* grad_f2 /* likewise, or NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* The PCA picture of a feature map (feature_visualization.py:84-101, plot_pca: sklearn PCA(n_components=3).fit(f).transform(f) on the (H W, C)
 * samples of a hooked layer or of the cross-attention maps, then the colouring) as two device ops (csrc/pca.hip).
 * gdf_op_pca: with x_p the C values of sample p, n samples, mu = sum_p x_p / n and cov = sum_p (x_p - mu)(x_p - mu)^T / (n - 1):
 *     components   the k leading eigenvectors v_1 .. v_k of cov, unit norm, each signed so that its entry of largest magnitude is positive
 *                  (the lowest channel among equal magnitudes): scikit-learn's svd_flip(u_based_decision=False)
 *     variance     their eigenvalues, descending;  total_variance = trace(cov);  projection[b, j, p] = <x_p - mu, v_j>
 *   src        one logical (B, C, H, W) tensor, fp16 (f32 = 0) or fp32, with element strides sb/sc/sy/sx, read only; `coff` is ignored.  A map with
 *              sx == 1 (NCHW, what gdf_op_aggregate writes) is read with lanes along the pixels; one with sc == 1, C a multiple of 8 (fp32: 4) and
 *              16-byte aligned pixels with 16-byte loads along C; any other strides are correct, not fast.
 *   joint      0: B independent PCAs, one per image (G = B, n = H W).  1: one PCA over the B H W pixels of the batch (G = 1), so that the images
 *              share their components.
 *   outputs    fp32: mean (G, C), components (G, k, C), variance (G, k), total_variance (G), projection (B, k, H, W) or NULL;
 *              info (G, 2) int32: the iterations used and 1 if converged, else 0.
 *   mean       fp32, compensated sums in a fixed order.
 *   covariance of the CENTRED values (never the Gram matrix minus n mu mu^T) on the MFMA units with fp32 accumulation: (x - mu) times a power of
 *              two is split into an fp16 (hi, lo) pair as it is staged, lo lo + lo hi + hi lo + hi hi; upper-triangular 128 x 128 tiles, mirrored, so cov
 *              is exactly symmetric; the samples are split over at most 64 workgroups per tile whose partial tiles are added in a fixed order
 *              (one fp32 accumulation chain covers at most 8192 samples up to n = 524 288 and n / 64 beyond: a joint run of more than 32
 *              128 x 128 images accumulates longer chains, which no test covers); C is padded to the tile
 *              with zeros the kernel writes.
 *   eigenpairs block subspace iteration with min(8, C) vectors from a fixed starting block, fp32; per iteration cov @ V over many workgroups, then
 *              one workgroup: the Rayleigh-Ritz step (an 8 x 8 Jacobi solve) and the orthonormalisation of the next block.  The PCA has converged
 *              when max_j ||cov v_j - lambda_j v_j|| <= tol lambda_1 over the k wanted pairs; tol = 2^-20 (16 fp32 roundings) and max_iter = 256
 *              are the Python defaults.  That criterion bounds an eigenvector's error by tol lambda_1 / gap only, so when it is first met, at
 *              iteration i, converged is reported and i / 2 + 2 further iterations take the residual to its fp32 floor; info counts them all.
 *              All max_iter iterations are enqueued as ordinary launches; after the last of those further iterations a device flag makes the
 *              remaining launches return at once.  A run that reaches max_iter before the criterion is met reports converged = 0 with the
 *              last Ritz pairs: not an error.  variance_j = <v_j, cov v_j> / <v_j, v_j> of the final vectors, accumulated in double, rounded
 *              once.  An eigenvalue that is not above 2^-20 lambda_1 cannot be told from rounding in fp32: that component is the zero vector
 *              with variance 0 (so a map whose third direction is exactly constant projects to exactly 0), and such a direction leaves the
 *              block.
 *   workspace  gdf_op_pca_workspace(B, C, H, W, k, joint) bytes, 16-byte aligned, caller-owned, contents undefined before and after: the padded
 *              covariance (G, Cpad, Cpad), the partial tiles and the blocks.
 * gdf_op_pca_rgb: projection (B, 3, H, W) fp32 contiguous -> out (B, OH, OW, 3) uint8: per component min and max over the image (over the batch
 * when joint), n = (p - min) / (max - min) in fp32, n * 255 truncated; output pixel (oy, ox) takes the source pixel floor((o + 0.5) in / out) of
 * each axis, clamped: Pillow's nearest resize.  A component of zero range is written as 0 (the reference casts NaN there).  The op has no
 * workspace, so every workgroup takes the min and max itself: with joint = 1 and B > 64 that is B * B * H * W reads.
 * No atomics, every reduction in a fixed order, no grid-wide wait: the same inputs give the same bits on any stream, and with joint = 0 at any
 * batch position.  Stream-ordered, nothing read back, no allocation.  A null required pointer, C, H or W below 1, B < 0, k outside 1 .. 8 or above
 * min(C, n - 1), max_iter outside 1 .. 1024, a tol that is negative or not finite, a misaligned or too small workspace: GDF_ERR_ARG before any
 * launch.  C > 4096, B > 65535, B * H * W >= 2^31: GDF_ERR_UNSUPPORTED.  B == 0 is a successful no-op. */
size_t gdf_op_pca_workspace(int B, int C, int H, int W, int k, int joint);
int gdf_op_pca(const gdf_agg_src* src, int B, int k, int joint, int max_iter, float tol, float* mean /* (G, C) */,
               float* components /* (G, k, C) */, float* variance /* (G, k) */, float* total_variance /* (G) */,
               float* projection /* (B, k, H, W) or NULL */, int* info /* (G, 2) */, void* workspace, size_t workspace_bytes, void* stream);
int gdf_op_pca_rgb(const float* projection /* (B, 3, H, W) */, int B, int H, int W, int joint, unsigned char* out /* (B, OH, OW, 3) */, int OH,
                   int OW, void* stream);
/* The label-scarce segmentation evaluator's second step on an aggregated map (scarce_segmentation/segmentation/pixel_classifier.py:70-107,
 * predict_labels): an ensemble of M per-pixel MLPs (pixel_classifier, :14-36) over every pixel, the per-pixel majority vote and the ensemble's
 * Jensen-Shannon uncertainty (csrc/pixcls.hip).  The networks are given BATCHNORM-FOLDED: eval-mode BatchNorm1d after ReLU is an
 * affine map and folds into the next Linear, so model m is  logits = W3 relu(W2 relu(W1 x + b1) + b2) + b3.
 *   gdf_pixcls_create   host fp32 arrays W1 (M, h1, C), b1 (M, h1), W2 (M, h2, h1), b2 (M, h2), W3 (M, K, h2), b3 (M, K), row-major as nn.Linear
 *                       stores them.  Uploads once; W1 and W2 are packed as an fp16 (hi, lo) pair per element, each row scaled by a power of two that
 *                       the kernel's fp32 epilogue undoes (the pair carries 22 bits of every weight).  Synchronous; the arrays may be freed afterwards.
 *                       M <= 16, K <= 64, h1 and h2 multiples of 32 up to 256, anything beyond: GDF_ERR_UNSUPPORTED; a null pointer or a size
 *                       below 1: GDF_ERR_ARG.
 *   gdf_pixcls_workspace  bytes of the workspace of one predict call on a (B, C, H, W) map; 0 for a null handle.
 *   gdf_pixcls_predict  x: a logical (B, C, H, W) tensor, fp16 (f32 = 0) or fp32, element strides sb/sc/sy/sx, read only, `coff` ignored; pixel
 *                       p = (b H + y) W + x.  sx == 1 (NCHW, what gdf_op_aggregate writes; the reference's (P, dim) view of it has strides (1, P))
 *                       is read with lanes along the pixels; sc == 1 with C a multiple of 8 (fp32: 4) and 16-byte aligned pixels (a channels-last
 *                       hook; the pixel may be longer than C) with 16-byte loads along C; any other strides are correct, not fast.
 *                       Layer 1 runs on the MFMA units with fp32 accumulation: an fp16 map is multiplied as given with W1's hi and lo halves, an
 *                       fp32 map is split into an fp16 (hi, lo) pair as it is loaded (hi hi + hi lo + lo hi; it must lie in the fp16 range).
 *                       Layer 2 runs on the MFMA units too, on the workgroup's hidden tile in LDS: hidden 1 as an fp16 (hi, lo) pair, W2 packed like
 *                       W1, three products; layer 3 is fp32 FMAs.  No hidden activation is ever a single 16-bit number; none reaches memory.
 *       logits          (M, B H W, K) fp32, or NULL: they are then kept in the workspace only
 *       model_labels    (M, B, H, W) uint8 or NULL: per model the LOWEST index among equal maxima
 *       js              (B, H, W) fp32 or NULL: H(mean_m softmax_m) - mean_m H(softmax_m) in fp32 with expf / logf; the mean is renormalised and its
 *                       entropy is -sum p log(clamp(p, eps, 1 - eps)), eps = 2^-23, as torch.distributions.Categorical(probs) computes it
 *       labels          (B, H, W) int64: the most frequent per-model label, the SMALLEST among equally frequent ones (torch.mode's rule)
 * Two launches, stream-ordered, no atomics, fixed summation order (the same inputs give the same bits on any stream), nothing read back, no
 * allocation.  A null pointer (handle, x, labels, workspace), H or W below 1, B < 0, x->C != C, a workspace that is not 16-byte aligned or smaller
 * than gdf_pixcls_workspace says: GDF_ERR_ARG before any launch.  B * H * W >= 2^31: GDF_ERR_UNSUPPORTED.  B == 0 is a successful no-op. */
typedef struct gdf_pixcls_s* gdf_pixcls;
int gdf_pixcls_create(int C, int M, int h1, int h2, int K, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                      const float* b3, gdf_pixcls* out);
void gdf_pixcls_destroy(gdf_pixcls h);
size_t gdf_pixcls_workspace(gdf_pixcls h, int B, int H, int W);
int gdf_pixcls_predict(gdf_pixcls h, const gdf_agg_src* x, int B, long long* labels /* (B, H, W) */, float* js /* (B, H, W) or NULL */,
                       uint8_t* model_labels /* (M, B, H, W) or NULL */, float* logits /* (M, B H W, K) or NULL */, void* workspace,
                       size_t workspace_bytes, void* stream);
/* The trained head of the correspondence evaluator on an aggregated map (correspondence/correspondence/aggregation_network.py:20-22, 97-100:
 * self.out = nn.Conv2d(dim, out_dim, kernel_size=3, stride=1, padding=1, bias=False); x = x.type(torch.float32); x = self.out(x); run on the
 * source and on the target map of every pair, task-corres.py:60-67):
 *   out[b, co, y, x] = bias[co] + sum_{ci, dy, dx} W[co, ci, dy, dx] in[b, ci, y + dy - 1, x + dx - 1],  zeros outside the image
 * (torch's cross-correlation: stride 1, padding 1, no dilation, no groups) as an implicit GEMM on the MFMA units (csrc/agghead.hip).
 *   gdf_agghead_create   host fp32 W (Cout, Cin, 3, 3) as nn.Conv2d stores it, bias (Cout) or NULL.  Uploads once: every weight becomes an fp16
 *                        (hi, lo) pair, each output channel's 9 Cin row scaled by a power of two that the fp32 epilogue undoes (the pair carries
 *                        22 bits of every weight), in MFMA fragment order, 8 bytes per weight (Cin padded to 32, Cout to 32) addressed with 64-bit
 *                        offsets: 7360 -> 3680 takes 975 MB of device memory.  Synchronous; the arrays may be freed afterwards.  An all-zero row
 *                        yields that row's bias.  A null W or out, Cin or Cout below 1, a weight or bias that is not finite: GDF_ERR_ARG.
 *   gdf_agghead_forward  x: a logical (B, Cin, H, W) tensor, fp16 (f32 = 0) or fp32, element strides sb/sc/sy/sx, read only, `coff` ignored.  sx == 1
 *                        (NCHW, what gdf_op_aggregate writes) is read with lanes along x; sc == 1 with C a multiple of 8 (fp32: 4) and 16-byte
 *                        aligned pixels (a channels-last hook; the pixel may be longer than C) with 16-byte loads along C; any other strides are
 *                        correct, not fast.  An fp16 map is multiplied as given with the hi and lo halves of W; an fp32 map is split into an fp16
 *                        (hi, lo) pair as it is staged (hi hi + hi lo + lo hi; it must lie in the fp16 range).  fp32 accumulation, folded into a
 *                        second fp32 total after every 32 input channels.  The padding is zeros the kernel writes: nothing beside the map is read.
 *       out              (B, Cout, H, W) fp32 contiguous, as the reference returns it
 * One launch, stream-ordered, no atomics, no workspace, fixed summation order; every workgroup's tile lies inside one image, so an image's bits depend
 * neither on B nor on its place in the batch, and the same inputs give the same bits on any stream.  A null pointer (handle, x, x->ptr, out), H or W
 * below 1, B < 0, x->C != Cin, B * H * W >= 2^31: GDF_ERR_ARG before any launch.  B == 0 is a successful no-op. */
typedef struct gdf_agghead_s* gdf_agghead;
int gdf_agghead_create(int Cin, int Cout, const float* W /* host, (Cout, Cin, 3, 3) */, const float* bias /* host (Cout) or NULL */, gdf_agghead* out);
void gdf_agghead_destroy(gdf_agghead h);
int gdf_agghead_forward(gdf_agghead h, const gdf_agg_src* x, int B, float* out /* (B, Cout, H, W) */, void* stream);
/* Training that head (correspondence/task-corres.py train(), `--algorithm conv`: loss.backward() through aggregation_network.out, then AdamW):
 * the weight gradient of the convolution and the repack of updated weights, both on the device (csrc/aggwgrad.hip, csrc/agghead.hip).
 *   gdf_agghead_wgrad    dW[co, ci, dy, dx] = sum_{b, y, x} grad_out[b, co, y, x] x[b, ci, y + dy - 1, x + dx - 1], zeros outside the image.
 *       x                the map the forward took: logical (B, Cin, H, W), fp16 or fp32, element strides sb/sc/sy/sx, read only, `coff` ignored;
 *                        read with its own strides, lanes along x (coalesced where sx == 1; a channels-last map is correct, not fast)
 *       grad_out         (B, Cout, H, W) fp32 contiguous: what gdf_op_clip_loss_backward writes
 *       dW               (Cout, Cin, 3, 3) fp32 contiguous, nn.Conv2d.weight's layout, addressed with 64-bit offsets.  accumulate = 0 writes it;
 *                        accumulate = 1 forms the complete sum first and adds it once to what dW holds, so dW0 + (accumulate = 0) and
 *                        (accumulate = 1 onto dW0) have the same bits
 *       ws               gdf_agghead_wgrad_workspace bytes, 16-byte aligned; afterwards it holds max |grad_out| per output channel (Cout floats)
 *                        and, 256-byte aligned behind them, the power-of-two shift used for that channel (Cout ints)
 *                        Arithmetic: grad_out becomes an fp16 (hi, lo) pair per element after a power-of-two scale per output channel that puts
 *                        the channel's maximum into [2^13, 2^14) (saturating; an all-zero channel yields exactly 0; the epilogue undoes the scale
 *                        exactly); an fp16 map is multiplied as given (lo x, hi x), an fp32 map is split as it is staged (lo lo dropped); fp32
 *                        accumulation on the MFMA units, folded into a second fp32 total every 128 pixels.  grad_out is not validated: a
 *                        non-finite value gives unspecified values in its output channel's rows of dW, never an access outside the buffers.
 *                        One pre-pass and one launch, stream-ordered, no atomics, no split-K, fixed summation order (the same inputs give the same
 *                        bits on any stream), no allocation.  A null pointer (x, x->ptr, grad_out, dW, ws), Cout, C, H or W below 1, B < 0,
 *                        B * H * W >= 2^31, a workspace that is too small or misaligned: GDF_ERR_ARG before any launch.  B == 0 is a successful
 *                        no-op that launches nothing: with accumulate = 0 it does NOT zero dW.
 *   gdf_agghead_update   overwrites the handle's packed fragment image and 1 / scale from W_dev, an fp32 OIHW (Cout, Cin, 3, 3) DEVICE tensor, by
 *                        gdf_agghead_create's rule (row maximum, sh = 13 - ilogb(max), hi = fp16(v 2^sh), lo = fp16(v 2^sh - hi), the same
 *                        fragment order, zeros in the padding): for finite weights the image is bit-identical to what gdf_agghead_create packs
 *                        on the host from the same values.  Two launches, stream-ordered after the forwards already queued on `stream`, no host
 *                        synchronisation, no allocation; the bias stays.  The weights are not validated (that would need a read-back).
 *   gdf_agghead_create_device   the allocation plus the same kernels; bias_dev (Cout) on the device or NULL.  Asynchronous on `stream`.
 * A null handle, W_dev or out, Cin or Cout below 1: GDF_ERR_ARG. */
size_t gdf_agghead_wgrad_workspace(int B, int Cin, int Cout, int H, int W);
int gdf_agghead_wgrad(const gdf_agg_src* x, int B, const float* grad_out /* (B, Cout, H, W) */, int Cout, float* dW /* (Cout, Cin, 3, 3) */,
                      int accumulate, void* ws, size_t ws_bytes, void* stream);
int gdf_agghead_create_device(int Cin, int Cout, const float* W_dev, const float* bias_dev, void* stream, gdf_agghead* out);
int gdf_agghead_update(gdf_agghead h, const float* W_dev, void* stream);
/* `feature_resize` (components/feature_extractor.py:51-53): adaptive_avg_pool2d to (OH, OW) = (H / r, W / r) (integer division) of a
 * channels-last hook (strides sb, 1, sy, sx; C % 8 == 0) -> (B, OH, OW, C) fp16, fp32 accumulation.  Output row o averages source rows
 * [floor(o H / OH), ceil((o + 1) H / OH)), columns likewise: the r x r window where r divides the size, otherwise longer windows that may
 * overlap and cover every row and column.  H < r or W < r is an error. */
int gdf_op_avg_pool(const void* src, long sb, long sy, long sx, int B, int C, int H, int W, int r, void* out, void* stream);
/* aggregated `attn` feature (components/attention.py:238-244, 141-161): mean over heads (rounded to fp16 like the
 * reference's `attention_probs.mean(1)`), then mean over the n <= 32 maps (B, heads, Q, K) fp16 of one (category, size)
 * group -> (B, Q, K) fp32; gdf_op_resize_concat then turns it into the (B, K, img/8, img/8) slice of the feature. */
int gdf_op_maps_mean(const void* const* maps, int n, int B, int heads, int Q, int K, float* out, void* stream);

/* ---- ControlNet conditioning (csrc/control.hip) ---- */

/* One launch of residual_add_kernel over n <= 16 tensors: dst[r][0..C) += res[r][0..C), r < rows — the skip and mid-block adds of
 * unet_2d_condition.py:1236-1245, 1269-1270, in place on the slices of the up-path concat buffers a UNet plan keeps its skips in.
 *   dst   fp16 rows of ld elements; the pointer carries the slice's column offset (ld >= C)
 *   lo    0: a plain image, dst = fp16(dst + res), one rounding.  > 0: dst is a split (hi, lo) pair, lo `lo` >= C elements after hi in the same
 *         row; the new pair is hi' = fp16(v), lo' = fp16(v - hi') of v = hi + lo + res in fp32
 *   res   fp16 contiguous [rows][C], read only
 * C, ld and lo are multiples of 8 and both pointers 16-byte aligned (16 bytes per lane); anything else is an error and nothing is launched.
 * Items with rows == 0 or C == 0 are skipped. */
typedef struct gdf_residual_add_item {
  void* dst; int ld; int lo;
  const void* res; int rows; int C;
} gdf_residual_add_item;
int gdf_op_residual_add(const gdf_residual_add_item* items, int n, void* stream);

/* One launch of cond_conv3x3_kernel (csrc/cond_embed.hip): a 3x3 convolution, padding 1, of the ControlNet conditioning embedding
 * (`controlnet_cond_embedding` of diffusers' ControlNetModel: conv_in, blocks.0..5, conv_out).
 *   x         NHWC fp16 [B][H][W][ldx >= Cin], read only
 *   w_packed  the weights as gdf_op_cond_pack_weights lays them out (gdf_op_cond_weight_bytes bytes): fp16 [k / 8][Cout][8] with
 *             k = tap * Cin + c, zero padded to a multiple of 32 in k
 *   bias      fp32 [Cout] or NULL
 *   out       NHWC fp16 [B][OH][OW][ldo >= Cout], OH = (H - 1) / stride + 1: out = fp16(act(acc + bias)) with fp32 accumulation, act = SiLU
 *             when silu != 0; add_into != 0: out = fp16(act(acc + bias) + out) (the sum of `conv_in(sample) + controlnet_cond_embedding(cond)`)
 * (Cin, Cout) is one of 8->16 (the 3-channel image packed to 8), 16->16, 16->32, 32->32, 32->96, 96->96, 96->256, 256->any multiple of 64;
 * stride 1 or 2, at 2 with even H and W; ldx and ldo multiples of 8, ldx >= Cin, ldo >= Cout; every pointer 16-byte aligned.  Anything else is
 * an error and nothing is launched.  Columns from Cout up of an out row are not written. */
int gdf_op_cond_conv3x3(const void* x, int B, int H, int W, int Cin, int ldx, const void* w_packed, const float* bias, int Cout, int stride,
                        int silu, void* out, int ldo, int add_into, void* stream);
/* OIHW weights (Cout, Cin_src <= Cin, 3, 3) of dtype src_dtype (0 fp16, 1 fp32, 2 bf16) -> the packed layout; input channels from Cin_src up
 * are zero (the first layer: Cin_src = 3, Cin = 8). */
size_t gdf_op_cond_weight_bytes(int Cin, int Cout);
int gdf_op_cond_pack_weights(const void* w_oihw, int src_dtype, void* dst, int Cout, int Cin_src, int Cin, void* stream);
/* control image NCHW (B, C <= 8, H, W), fp16 (GDF_F16) or fp32 (GDF_F32) -> NHWC pixels of 8 fp16 channels, channels from C up zero. */
int gdf_op_cond_pack_image(const void* x_nchw, int src_dtype, int B, int C, int H, int W, void* nhwc8, void* stream);

/* ---- Canny edge detector on the device (csrc/canny.hip): the preprocessor of the 'canny' / 'canny-xl' ControlNets, OpenCV 4.x
 * cv::Canny(src8u, low, high, apertureSize = 3, L2gradient = false) restated in integer arithmetic.  Stream-ordered, caller-owned
 * buffers, no device -> host read; the number of launches depends on nothing but the entry called.
 *   src_kind  GDF_CANNY_U8_HWC3  uint8 [B][H][W][3] (np.array of an RGB PIL image)      GDF_CANNY_U8_HW  uint8 [B][H][W]
 *             GDF_CANNY_F32_NCHW / GDF_CANNY_F16_NCHW  [B][3][H][W] in [-1, 1], quantised on load as the reference's restore_from_tensor_to_image
 *             does: to fp32, rint(clamp(x / 2 + 0.5, 0, 1) * 255), half to even
 *   low, high the thresholds (swapped when low > high); a pixel is examined when its magnitude > low, strong when > high
 *   cls       uint8 [B][H][W], OpenCV's map values: 2 strong, 0 candidate (kept by the non-maximum suppression, not strong), 1 neither
 *   dst_kind  GDF_CANNY_DST_U8  uint8 [B][H][W] 0 / 255 (cv2's output)      GDF_CANNY_DST_F16_NCHW3  fp16 [B][3][H][W] 0.0 / 1.0: the control tensor of
 *             the three-channel edge image
 *   workspace gdf_op_canny_workspace_bytes(B, H, W) bytes, the caller's; nothing is kept in it between calls
 * H, W >= 1 (1 x 1 is legal); B H W < 2^31 (32-bit labels), anything larger is GDF_ERR_UNSUPPORTED; src 4-byte, cls / dst / workspace 16-byte aligned.
 * gdf_op_canny_link takes any class map (values 0 / 1 / 2), also ones no image produces; gdf_op_canny = classify into the workspace, then link. */
enum { GDF_CANNY_U8_HWC3 = 0, GDF_CANNY_U8_HW = 1, GDF_CANNY_F32_NCHW = 2, GDF_CANNY_F16_NCHW = 3 };
enum { GDF_CANNY_DST_U8 = 0, GDF_CANNY_DST_F16_NCHW3 = 1 };
size_t gdf_op_canny_workspace_bytes(int B, int H, int W);
int gdf_op_canny_classify(const void* src, int src_kind, int B, int H, int W, int low, int high, void* cls, void* stream);
int gdf_op_canny_link(const void* cls, int B, int H, int W, void* dst, int dst_kind, void* workspace, void* stream);
int gdf_op_canny(const void* src, int src_kind, int B, int H, int W, int low, int high, void* dst, int dst_kind, void* workspace, void* stream);

/* ---- PIL-to-tensor preprocessing on the device (csrc/preproc.hip): preprocess_image of one PIL image,
 * pipe.image_processor.preprocess(img.resize((S, S)).convert("RGB")), i.e. Pillow's ImagingResample (8 bits per channel, BICUBIC, whole-image box)
 * restated in its own fixed-point arithmetic, equal to Pillow byte for byte.  Stream-ordered, caller-owned buffers, no device -> host
 * read and no host synchronisation; every argument is checked before the first launch.
 *   gdf_op_pil_coeffs   one axis' table for `in` source and `out` target samples, made on the device in IEEE double without fused multiply-add:
 *                       bounds int32 [out][2] = (xmin, xmax), kk int32 [out][*ksize] (2^22 fixed point, entries from xmax up zero); *ksize (host) =
 *                       2 ceil(2 max(in / out, 1)) + 1.  One launch.
 *   gdf_op_pil_resize_u8  src uint8 [src_h][src_w][channels], channels 1 (mode L) or 3 (mode RGB), ANY byte alignment ->
 *                       dst_u8_hwc3  uint8 [out_h][out_w][3] = np.array(Image.fromarray(src).resize((out_w, out_h)).convert("RGB")), and / or
 *                       dst_f32_chw  fp32 [3][out_h][out_w] = (fp32(u) / 255) * 2 - 1 of those bytes: one row of the (B, 3, S, S) batch
 *                       (either may be NULL, not both).  Horizontal pass first into a uint8 intermediate, then vertical; a pass whose axis already
 *                       has the target size is skipped, with both skipped the bytes pass through.  At most four launches.
 *   workspace           gdf_op_pil_resize_workspace_bytes(...) bytes (0 for arguments gdf_op_pil_resize_u8 refuses), 16-byte aligned: the two
 *                       tables and the intermediate; nothing is kept in it between calls
 * Sizes >= 1 (1 x 1 is legal).  in / out > 32 on an axis (ksize > 129) and 2^31 bytes or more in a buffer are GDF_ERR_UNSUPPORTED; every other
 * refused argument is GDF_ERR_ARG. */
int gdf_op_pil_coeffs(int in, int out, void* bounds, void* kk, int* ksize, void* stream);
size_t gdf_op_pil_resize_workspace_bytes(int src_h, int src_w, int channels, int out_h, int out_w);
int gdf_op_pil_resize_u8(const void* src, int src_h, int src_w, int channels, int out_h, int out_w, void* dst_u8_hwc3, void* dst_f32_chw,
                         void* workspace, void* stream);

/* ---- MMDiT (Flux) kernels (reference files cited in csrc/dit.hip, gdf_flux.h) ---- */

/* Element type of the 16-bit operands ("e16": A, W, out16, q/k/v/o, y) of the MMDiT entry points below, per calling thread:
 * GDF_F16 (default) or GDF_BF16 (what a gdf_flux_desc.compute_dtype = GDF_BF16 model runs).  aux16 (a hook) is always fp16. */
int gdf_op_set_e16(int dtype);

/* Dense GEMM with the MMDiT epilogue: v = A W^T + bias; act=1: tanh-GELU; vec != NULL: v = vec_mul ? v * vec[s] : v + vec[s]
 * (s = row / rps for row < seg_rows or seg_rows == 0, else (row - seg_rows) / rps2; vec fp32 rows of ldvec);
 * aux16 (optional) receives fp16(v) BEFORE the gate; then + res32, stores out16 / out32.
 * Replaces nn.Linear + gate/residual arithmetic of transformer_flux.py:95-106, 191-218. */
/* 'fp8-mx' MMDiT plans (gdf_flux.h, GDF_FP8MX; opt-in, LOWER precision than the reference's bf16): 16-bit rows -> OCP e4m3 bytes with one
 * power-of-two scale per row, q = fp8(v / scale[r]) (activations per token, weights per output channel), and the GEMM on such operands:
 * out = act((A8 W8^T) * a_scale[row] * w_scale[col] + bias) (+ res32), v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (the
 * per-row / per-channel scales are applied to the fp32 accumulators), bf16 out16.  K % 128 == 0; 256x256 tiles.
 * Replaces the same nn.Linear call sites as gdf_op_gemm_dit (transformer_flux.py:86-112, 167-226). */
int gdf_op_quant_rows_fp8(const void* x16, int ld, int R, int K, int src_bf16, void* q8, int ldq, float* scale, void* stream);
int gdf_op_gemm_mx(const void* A8, int lda, const float* a_scale, const void* W8, const float* w_scale, const float* bias, int act,
                   const float* res32, int ldres, void* out16, int ldo16, float* out32, int ldo32, int M, int N, int K, void* stream);

int gdf_op_gemm_dit(const void* A, int lda, const void* W, const float* bias, int act, const float* vec, int ldvec, int vec_mul,
                    int rps, int seg_rows, int rps2, const float* res32, int ldres, void* aux16, int ldaux, void* out16,
                    int ldo16, float* out32, int ldo32, int M, int N, int K, int variant, void* stream);

/* y = LayerNorm(x, eps, no affine) * (1 + scale[s]) + shift[s]  (AdaLayerNormZero & co.); x fp32 [R][ld], y fp16 [R][C]. */
int gdf_op_layernorm_mod(const float* x32, int ld, int R, int C, float eps, const float* scale, const float* shift, int ldm,
                         int rps, int seg_rows, int rps2, void* y, void* stream);

/* The same kernel with every argument of its launcher (test surface): exactly one of x16 (fp16, whatever `bf16` says) / x32 is the source,
 * rows of ld elements (ld % 8 == 0 / ld % 4 == 0); y fp16 (bf16 = 0) or bf16 rows of ldy elements (0: C); y_lo > 0: y is a split pair, hi at
 * column 0 and lo = e16(v - hi) at column y_lo ('bfloat16x2' plans); q8 != NULL: the same row also as OCP e4m3 bytes, rows of ldq8, with one
 * power-of-two scale per row in q8_scale, both made from the fp32 values ('fp8-mx' plans, see gdf_op_quant_rows_fp8). */
int gdf_op_layernorm_mod_ex(const void* x16, const float* x32, int ld, int R, int C, float eps, const float* scale, const float* shift,
                            int ldm, int rps, int seg_rows, int rps2, void* y, int bf16, int ldy, int y_lo, void* q8, int ldq8,
                            float* q8_scale, void* stream);
/* Host arithmetic only: the MAXC of the layernorm_mod_kernel<MAXC> (8 * 64 * MAXC columns in registers) the launcher instantiates for C
 * columns: 1, 2, 4, 6 or 8; 0 where it rejects C (C % 8 != 0, C > 4096). */
int gdf_op_layernorm_mod_path(int C);

/* In place RMSNorm(q), RMSNorm(k) per head (D = 128) + rotary embedding on fp16 rows [R][ld]; position = pos0 + r % rps. */
int gdf_op_qk_norm_rope(void* x, int ld, int R, int heads, int q_col, int k_col, const float* wq, const float* wk, float eps,
                        const float* cos_t, const float* sin_t, int pos0, int rps, void* stream);

/* FluxPosEmbed: ids fp32 [S][3] -> cos/sin fp32 [S][axes0+axes1+axes2] written at row offset row0. */
int gdf_op_rope_table(const float* ids, int S, int a0, int a1, int a2, float* cos_t, float* sin_t, int row0, void* stream);

/* Joint attention over [T text | S image] tokens per sample, rows region-major [B*T text rows][B*S image rows]. */
int gdf_op_attention_joint(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, int B,
                           int heads, int T, int S, int D, void* stream);

/* One launch of latent_step_kernel: the scheduler update between two forwards of a latent trajectory (gdf_trajectory, gdf.h).
 *   latents_f32  (B, 4, H, W) fp32 NCHW master, updated in place:  x' = c_sample * x + c_eps * eps
 *   noise_pred   (B, H, W, 4) fp16 channels-last (what gdf_forward writes); read only
 *   latents_f16  (B, 4, H, W) fp16 NCHW out:  c_in[next] * x'   (the scheduler's scale_model_input for the next forward)
 *   timesteps    (B) fp32 out: the next row's timestep in every slot
 *   steps        device block  int32 {step, ticket, n_rows, 0}  followed by  float rows[n_rows][4] = {timestep, c_in, c_sample, c_eps};
 *                ticket must be 0 before the first launch.  The launch uses row `step` for the update and row min(step + 1, n_rows - 1)
 *                ("next") for c_in and the timestep, then stores step + 1: consecutive steps are the same launch with the same arguments.
 *                A step outside [0, n_rows) writes nothing.
 *   prime = 1    no update: eps is not read and the master is not written; row 0 is "next" and step becomes 0 (the launch in front of the
 *                first forward).
 * Replaces the latent update of /root/reference/feature/components/ddim_inversion.py:39-41. */
int gdf_op_latent_step(float* latents_f32, const void* noise_pred, void* latents_f16, float* timesteps, void* steps, int B, int H, int W,
                       int prime, void* stream);

/* One launch of guided_step_kernel: the update between two forwards of a guided sampling run (gdf_sample, gdf.h) — classifier-free
 * guidance, a scheduler step with up to five model outputs of history, and the next forward's input.  B counts the samples of the master;
 * a guided run's forwards have batch 2B.
 *   latents_f32  (B, 4, H, W) fp32 NCHW master, updated in place
 *   noise_pred   fp16 channels-last, read only: guided (2B, H, W, 4) with rows [0, B) unconditional and [B, 2B) conditional — the order of
 *                torch.cat([negative, positive]) —, unguided (B, H, W, 4)
 *   history      (5, B, 4, H, W) fp32: ring of the last five combined noise predictions; step k writes slot k mod 5
 *   latents_f16  fp16 NCHW out, c_in[next] * x': guided (2B, 4, H, W), the same values in both halves; unguided (B, 4, H, W)
 *   timesteps    fp32 out, 2B (guided) or B entries: the next row's timestep in every slot
 *   steps        device block  int32 {step, ticket, n_rows, guided}, float g, three unused 32-bit words, then
 *                float rows[n_rows][8] = {timestep, c_in, c_sample, w0, w1, w2, w3, w4};  ticket must be 0 before the first launch
 * Step k, all in fp32:  e = e_u + g (e_c - e_u)  (unguided: e = noise_pred);  history[k mod 5] = e;
 *                       x' = c_sample x + sum_{j<5} w_j history[(k - j) mod 5];  a term with w_j == 0 is skipped, so a slot no step has
 * written is never read.  Row min(step + 1, n_rows - 1) supplies c_in and the timestep; then step + 1 is stored.  A step outside
 * [0, n_rows) writes nothing.  prime = 1: no update (noise_pred and history untouched, the master not written), row 0 supplies c_in and
 * the timestep, step becomes 0.
 * Replaces, per UNet call, the guidance combine, `scheduler.step` and `scheduler.scale_model_input` of a text-to-image loop such as the
 * reference's generate_with_extraction.py. */
int gdf_op_guided_step(float* latents_f32, const void* noise_pred, float* history, void* latents_f16, float* timesteps, void* steps, int B,
                       int H, int W, int prime, void* stream);

#ifdef __cplusplus
}
#endif
#endif
