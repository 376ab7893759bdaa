// Internal launch interface of the gfx950 kernels (C++ linkage; not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "../../include/gdf.h"    // GDF_MAX_TIMESTEPS
#include "launch.h"

typedef _Float16 half_t;

namespace gdf {

// One-time raise of a kernel's dynamic-LDS limit, per (kernel, device): `mask` is a static of the calling launcher with one
// bit per device ordinal.  Thread-safe without a lock — several extractors may run in threads of one process, one per
// device (reference correspondence/correspondence/aggregation_network.py:67-95); two racing first launches both set the
// attribute, which is idempotent.
inline hipError_t ensure_dyn_smem(std::atomic<uint64_t>& mask, const void* fn, int bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (mask.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return e;
  mask.fetch_or(bit, std::memory_order_release);
  return hipSuccess;
}

// ---- 16-bit element type of the MMDiT (Flux) path --------------------------------------------------------------------
// The reference runs Flux in torch.bfloat16 (components/models.py:158-169): real FLUX.1-dev activations leave the fp16 range.
// A model created with compute_dtype = GDF_BF16 keeps weights, activations and MFMA operands in bf16 (`half_t` is then only
// the 16-bit container); hooks stay fp16 like the reference's (feature_extractor.py:59-60), written with SATURATING casts.
#if defined(__HIPCC__)
__device__ __forceinline__ float e16_to_f32(half_t h, int bf) {
  return bf ? __uint_as_float((uint32_t)__builtin_bit_cast(unsigned short, h) << 16) : (float)h;
}
__device__ __forceinline__ half_t f32_to_e16(float v, int bf) {          // round to nearest even in both formats
  return bf ? __builtin_bit_cast(half_t, (__bf16)v) : (half_t)v;
}
__device__ __forceinline__ half_t f32_to_f16_sat(float v) {              // fp16 with saturation instead of +-inf (NaN stays NaN)
  // (v_med3_f32 alone answers min3 for a NaN operand, i.e. -65504: the NaN is passed round it)
  return (half_t)(v != v ? v : __builtin_amdgcn_fmed3f(v, -65504.0f, 65504.0f));
}
#endif

// ------------------------------------------------------------------------------------------------
// MFMA GEMM / implicit-GEMM convolution:  D[M,N] = A[M,K] * Wt[N,K]^T  (+ fused epilogue)
// ------------------------------------------------------------------------------------------------
enum { A_DENSE = 0, A_CONV3 = 1, A_CONV_SMALLC = 2 };

struct GemmParams {
  // ---- A operand (fp16). DENSE: row-major [M][K] with leading dimension lda (elements).
  //      CONV3: NHWC activation [B][H][W][lda>=Cin]; rows of the GEMM are output pixels.
  const half_t* A;
  int lda;
  uint32_t a_bytes;      // extent of A in bytes (buffer bounds: loads past it return 0)
  int M, N, K;           // K = Cin (dense) or 9*Cin (conv3)
  int mode;
  int H, W;              // source spatial size (conv)
  int OH, OW;            // output spatial size (conv)
  int stride;            // 1 or 2 (conv)
  int ups;               // 1: source is nearest-upsampled x2 before the conv (Upsample2D fused)
  int pad0;              // 0: zero padding 1 on every side; 1: pad right / bottom only (F.pad (0,1,0,1), Downsample2D padding=0)
  int Cin;
  // ---- B operand: weights [N][K] fp16, K contiguous (conv3: K index = ((c / 64) * 9 + tap) * 64 + c % 64, launch_relayout_conv cblk = 64)
  const half_t* Wt;
  uint32_t w_bytes;
  // ---- epilogue:  v = acc + bias[col] + rowvec[row / rows_per_sample][col]
  //                 aux16 = fp16(v)                       (pre-residual copy: `res-increment` hook)
  //                 v += res32|res16[row][col]
  //                 out16 = fp16(v), out32 = v
  //      GEGLU: columns come in [32 h | 32 gate] groups; out col = h * gelu(gate), N_out = N/2
  const float* bias;
  const float* rowvec;
  int rows_per_sample;
  int ldrv;
  const float* res32;
  const half_t* res16;
  int ldres;
  half_t* out16;
  int ldo16;
  float* out32;
  int ldo32;
  half_t* aux16;
  int ldaux;
  int geglu;             // != 0: weight rows / bias are interleaved [16 h | 16 gate]; out = (h) * gelu(gate), N_out = N/2
  int bn;                // 128 (default) or 16 (very narrow N, e.g. conv_out)
  int splitk;            // > 1 (2-stage ring tiles, batch <= 1): blockIdx.y selects one of `splitk` contiguous K ranges; the launch then
                         // writes RAW fp32 partial sums to out32 + blockIdx.y * o32_sstride and launch_gemm_splitk() finishes the epilogue
  long o32_sstride;      // elements between consecutive partial-sum slabs
  int batch;             // > 1: blockIdx.y selects one of `batch` independent problems sharing A (grouped text-K/V projections)
  long w_bstride;        // elements between consecutive weight matrices
  long o_bstride;        // elements between consecutive out16 matrices
  int sb_gm, sb_gn;      // (set by launch_gemm) tiles per XCD super-block, 0 = linear XCD-chunked order
  int no_superblock;     // diagnostics: force the linear order
  int no_early_mma;      // diagnostics: disable the opposite-order heads of the two waves sharing a SIMD (256x128 variant)
  int variant;           // 0 = auto, else a tile forced by its public code (include/gdf_ops.h gdf_op_gemm; decoded in gemm.hip: unet_tile / dit_tile)
  // ---- MMDiT epilogue (dit != 0 selects gemm_dit_kernel; dense only) ----
  //      v = acc + bias;  act == 1: v = gelu_tanh(v);  rowvec: v = rv_mul ? v * rowvec[sample][col] : v + rowvec[sample][col];
  //      then residual / stores as above.  sample = row / rows_per_sample for row < rv_seg_rows (or rv_seg_rows == 0),
  //      else (row - rv_seg_rows) / rv_rps2  (joint stream laid out [all text rows][all image rows]).
  int dit;
  int act;
  int rv_mul;
  int rv_seg_rows, rv_rps2;
  int rv_tok;            // 1: the row vector is per TOKEN (row % rows_per_sample), e.g. the PatchEmbed positional table
  // MMDiT QKV projection (dit only, 256x256 tile: one 128-wide head per wave tile): RMSNorm over each 128-column head of the
  // q columns [0, qkn_nq) and the k columns [qkn_nq, 2 qkn_nq), then the rotary embedding of the row's position
  // (Attention.norm_q / norm_k + apply_rotary_emb, attention_processor.py:2300-2335), applied to the fp32 accumulators
  int qkn_nq;            // 0 = off
  const float* qkn_wq; const float* qkn_wk; float qkn_eps;
  const float* rope_cos; const float* rope_sin;      // [position][128]
  int qkn_pos0, qkn_rps;                             // position of row r: qkn_pos0 + r % qkn_rps           (r <  qkn_seg_rows or no segment)
  int qkn_seg_rows, qkn_pos1, qkn_rps2;              //                    qkn_pos1 + (r - seg_rows) % rps2  (r >= qkn_seg_rows > 0)
  int bf16;              // dit only: A, Wt and out16 are bf16 (mfma_f32_16x16x32_bf16); aux16 (a hook) stays fp16, saturating
  // fp16 RANGE control (VAE encoder: the stock SDXL VAE's residual stream leaves the fp16 range, the reference upcasts it to
  // fp32).  v = acc * acc_scale + bias ...; out16 = fp16(v * out16_scale).  A tensor whose fp16 image is stored with
  // out16_scale = 2^-k is read back by its consumer GEMM with acc_scale = 2^k (exact: powers of two).  0 means 1.
  float acc_scale, out16_scale;
  // SPLIT OPERANDS ("precise" plans, gdf_plan_opts.precise): an activation is stored as two fp16 numbers hi = fp16(v), lo = fp16(v - hi)
  // (22 mantissa bits) and the contraction runs over [hi | lo] against [W | W]:  A.W = hi.W + lo.W with K doubled, the weights read
  // twice from the SAME matrix.  k_w > 0: K of the weight matrix (K == 2 k_w); K-tile kt >= k_w / 64 of A starts a_lo_bytes after the
  // hi columns (conv3: per pixel) and reads weight K-tile kt - k_w / 64.  o16_lo > 0: out16 is written as such a pair, lo at
  // out16 + o16_lo elements (same row).  0 everywhere = plain fp16 operands (the default plans).
  int k_w;
  uint32_t a_lo_bytes;
  int o16_lo;
  // CU PARTITION (gdf_plan_opts.reserved[2]): > 0 = the launch stream is restricted to this many CUs (a CU-masked stream,
  // gdf_stream_create_cu_mask): tile selection, persistent grids and the XCD super-block order count workgroup slots on `cus`
  // CUs instead of the whole chip.  0 = the whole device.
  int cus;
  // MMDiT 'bfloat16x2' plans (gdf_flux_desc.compute_dtype = GDF_BF16X2): a bf16 kernel (dit, bf16) that stores out16 as SATURATING fp16 — the
  // q / k / v buffer of the attention kernel, whose internals run in fp16 in that mode (q, k are RMS-normalised, v is a linear of a
  // normalised tensor: inside the fp16 range by construction; 11 mantissa bits instead of 8)
  int out_f16;
  // MMDiT 'fp8-mx' plans: A and Wt hold fp8 (OCP e4m3) bytes — lda, K, a_bytes, w_bytes are given in 2-BYTE units exactly as for a 16-bit matrix
  // of half the width (a K-tile is 128 bytes either way) — multiplied with v_mfma_scale_f32_16x16x128_f8f6f4; the operands' power-of-two
  // scales are undone on the fp32 accumulators: acc * mx_rowscale[row] * mx_colscale[col] (either may be null = 1)
  int mx;
  const float* mx_rowscale;
  const float* mx_colscale;
  // GROUPNORM STATISTICS FROM THE PRODUCER (VAE op programs; 3x3 convs on the tiles gemm_gn_slab_rows() accepts): besides storing
  // out16, the epilogue sums x and x^2 of the stored values (v * out16_scale) per output channel over slabs of gemm_gn_slab_rows()
  // consecutive rows and writes them as gn_partial[(row / slab_rows) * N + c][2] — the layout launch_gn_finalize() reads, so the
  // GroupNorm that consumes the tensor needs no statistics pass of its own (a full HBM read of a 1-4 GB tensor at 1024^2).
  // Requires M % slab_rows == 0 and (rows per sample) % slab_rows == 0.  nullptr = off (every UNet / MMDiT plan).
  float* gn_partial;
};
// Dispatch: gemm_select() maps the parameters to a descriptor, which spells ONE instantiation (the template arguments of gemm_body); launch_gemm()
// launches the instantiation the descriptor names and gemm_kernel_name() prints the same descriptor.  Host arithmetic only, no pointer is followed.
struct GemmSel {
  bool ok;                 // false: launch_gemm refuses these parameters
  int MODE, BM, BN, STAGES; bool GEGLU, DIT, BF, QKN, SPLIT, MX, GNS;
  bool forced_missing;     // `variant` named a tile this form has no instantiation of: the descriptor is the form's 128x128 tile, which launch_gemm
                           // runs; gdf_op_gemm_ex and gdf_op_gemm_kernel refuse these
};
GemmSel gemm_select(const GemmParams& p);
hipError_t launch_gemm(const GemmParams& p, hipStream_t s);
// kernel symbol (as the profiler prints it) of the descriptor's instantiation, nullptr where !ok
const char* gemm_kernel_name(const GemmSel& k);
inline const char* gemm_kernel_name(const GemmParams& p) { return gemm_kernel_name(gemm_select(p)); }
// rows per statistics slab if launch_gemm can run `p` (shape, mode, epilogue form) with gn_partial set, else 0
int gemm_gn_slab_rows(const GemmParams& p);
// true when an MMDiT GEMM of this shape runs on the 256x256 tile, i.e. may carry the fused RMSNorm + RoPE epilogue (qkn_*)
bool gemm_qkn_ok(int M, int N, int K);
// Deterministic split-K for problems with few output tiles and a long K (the 8x8-level 3x3 convs of SD1.5: 160 tiles of 128x128,
// K = 11520..23040): gemm_splitk_factor() > 1 says it pays; the caller provides `splitk * M * N` floats of workspace, the GEMM
// launch writes one raw partial-sum slab per K range and splitk_reduce_kernel sums them in a fixed order and applies the epilogue.
int gemm_splitk_factor(const GemmParams& p);
hipError_t launch_gemm_splitk(const GemmParams& p, int splitk, float* ws, hipStream_t s);
// the first launch of launch_gemm_splitk as GemmParams `g` (host arithmetic): false where the split launch is refused; `splitk` is clamped to
// the K-tile count, <= 1 afterwards = the plain launch of `p`
bool gemm_splitk_pass1(const GemmParams& p, int& splitk, float* ws, GemmParams& g);

// ------------------------------------------------------------------------------------------------
// flash attention (self / cross), fp16 in, fp32 softmax, fp16 out
//   q: rows (b*Sq + i), head h at columns [h*D, h*D+D) with leading dim ldq; same for k, v, o.
// ------------------------------------------------------------------------------------------------
struct AttnParams {
  const half_t* q; int ldq;
  const half_t* k; int ldk;
  const half_t* v; int ldv;
  half_t* o; int ldo;
  int B, heads, Sq, Sk, D;
  int kv_bstride;        // rows between consecutive samples' K/V (Sk normally; 0 = all samples share one K/V set)
  float scale;
  half_t* map;           // optional: attention probabilities (B, heads, Sq, Sk) fp16 ('-map' hooks); seg_T > 0: `self-map`
  half_t* map2;          // seg_T > 0 only: `cross-map` (B, heads, Sq - seg_T, seg_T) (image queries x text keys)
  const int* kv_len;     // optional [B]: keys [kv_len[b], Sk) of sample b are masked out (prefix text mask)
  int seg_T;             // > 0: MMDiT joint sequence, region-major rows [B x seg_T text][B x (Sq - seg_T) image] (Sq == Sk)
  int bf16;              // D = 128 only: q, k, v, o are bf16 (mfma_f32_32x32x16_bf16, P rounded to bf16); maps stay fp16
  int o_lo;              // > 0 ("precise" plans): o is written as a split (hi, lo) pair, lo at o + o_lo elements in the same row
  int o_pair_bf16;       // with o_lo > 0 and fp16 q / k / v (bf16 == 0): the pair is written as bf16 hi + bf16 lo (MMDiT 'bfloat16x2' plans)
  int q_lo, kv_lo;       // both > 0 (full-split plans, fp16 UNet attention with 40 <= D <= 80): q, k and v are split (hi, lo) pairs, lo at +q_lo (q) /
                         // +kv_lo (k, v) elements in the same row; the kernel contracts over both halves (attn_kernel<..., QKP>).  Other head dims
                         // read the hi halves only.
  float o_scale;         // != 0: o is stored multiplied by this power of two (MMDiT 'float16s' plans: the [attn | mlp] operand rows of the single
                         // blocks share ONE fp16 range scale, undone on the consuming GEMM's accumulators)
};
hipError_t launch_attention(const AttnParams& p, hipStream_t s);
// kernel symbol launch_attention would pick (host arithmetic only: no pointer is dereferenced, no device call; only whether map / map2 / kv_len are
// set is read), nullptr for parameters it rejects.  Built from the descriptor the launch itself switches on.
const char* attention_kernel_name(const AttnParams& p);

// ------------------------------------------------------------------------------------------------
// normalisation / elementwise
// ------------------------------------------------------------------------------------------------
// Statistics are one-pass fp32 sums of x and x^2 per thread (double across threads / slabs): the error of rstd grows with (mean / std)^2 of a
// group and stays inside the fp16 output tolerance (1e-3) up to mean / std of about 32 (rstd off by <= 1e-4 there, 2e-3 at 128; DESIGN.md 3.3, tests/test_gpu_groupnorm.py).
// GroupNorm over NHWC rows x [B][HW][ld] (C channels used, G groups).  Two launches:
//   gn_stats : per-(sample, channel) affine table ab[b][c] = (rstd*gamma, beta - mean*rstd*gamma)
//              (`partial` is scratch of gn_partial_floats(B, HW, C) floats)
//   gn_apply : y = act(x*a + b) as contiguous fp16 [B*HW][C]; silu=1 applies v*sigmoid(v)
size_t gn_partial_floats(int B, int HW, int C);
// pixel rows per statistics slab of launch_gn_stats (its `partial` is [B][ceil(HW / slab)][C][2])
int gn_stats_slab(int B, int HW);
// split operands ("precise" plans): x_lo > 0 = the fp16 source is a (hi, lo) pair with lo x_lo elements after hi in the row;
// y_lo > 0 = y is written as such a pair (rows of ldy elements, lo at column offset y_lo); ldy = 0 means C
hipError_t launch_gn_stats(const half_t* x16, const float* x32, int ld, int B, int HW, int C, int G, float eps,
                           const float* gamma, const float* beta, float* partial, float* ab, hipStream_t s, int x_lo = 0);
hipError_t launch_gn_apply(const half_t* x16, const float* x32, int ld, int B, int HW, int C,
                           const float* ab, int silu, half_t* y, hipStream_t s, int x_lo = 0, int ldy = 0, int y_lo = 0);
// the second stage of launch_gn_stats alone: `partial` = [B][nslab][C][2] per-slab channel sums (sum x, sum x^2) produced by a GEMM
// epilogue (GemmParams::gn_partial) -> ab
// `fold`: scratch of gn_fold_floats(B, nslab, C) floats (0 = none needed) for the pre-reduction of many short slabs
size_t gn_fold_floats(int B, int nslab, int C);
hipError_t launch_gn_finalize(const float* partial, int nslab, int B, int HW, int C, int G, float eps, const float* gamma,
                              const float* beta, float* ab, float* fold, hipStream_t s);
// single-launch GroupNorm (+SiLU) for small feature maps; gn_fused_slab(...) != 0 says whether it applies
int gn_fused_slab(int B, int HW, int C, int G);
hipError_t launch_gn_fused(const half_t* x16, const float* x32, int ld, int B, int HW, int C, int G, float eps, const float* gamma,
                           const float* beta, int silu, half_t* y, hipStream_t s, int x_lo = 0, int ldy = 0, int y_lo = 0);
// LayerNorm over the last dim (C), rows x [R][ld]; y contiguous fp16 [R][C]
hipError_t launch_layernorm(const half_t* x16, const float* x32, int ld, int R, int C, float eps,
                            const float* gamma, const float* beta, half_t* y, hipStream_t s, int ldy = 0, int y_lo = 0);
// LayerNorm without affine + adaLN modulation (AdaLayerNormZero / ZeroSingle / Continuous and the norm2 modulate of
// the MMDiT blocks): y = LN(x, eps) * (1 + scale[s][c]) + shift[s][c]; s = row / rps for row < seg_rows (or
// seg_rows == 0), else (row - seg_rows) / rps2.  x fp32 (or fp16) [R][ld], y fp16 [R][C], scale/shift fp32 rows of ldm.
// y_lo > 0: y is written as a split pair (rows of ldy elements, hi at column 0, lo = e16(v - hi) at column y_lo)
// Exactly one of x16 / x32 is set.  x16 is ALWAYS fp16 (the kernel reads it with a plain cast whatever `bf16` says; `bf16` is the type of y
// only); no plan passes x16.  ld % 4 == 0 for x32, ld % 8 == 0 for x16 (16-byte loads).
hipError_t launch_layernorm_mod(const half_t* x16, const float* x32, int ld, int R, int C, float eps, const float* scale,
                                const float* shift, int ldm, int rps, int seg_rows, int rps2, half_t* y, hipStream_t s,
                                int bf16 = 0, int ldy = 0, int y_lo = 0, unsigned char* q8 = nullptr, int ldq8 = 0, float* q8_scale = nullptr);
// MAXC of the layernorm_mod_kernel<MAXC> that launch_layernorm_mod instantiates for C columns (1, 2, 4, 6, 8), or 0 where it rejects C
int layernorm_mod_maxc(int C);
// 'fp8-mx' plans: 16-bit rows [R][ld] (K columns) -> fp8 e4m3 [R][ldq] with one power-of-two scale per row (q = fp8(v / scale[r])).
// launch_layernorm_mod's q8 / q8_scale write the same form of its own output in the same pass.
hipError_t launch_quant_rows_fp8(const half_t* x, int ld, int R, int K, int bf16, unsigned char* q, int ldq, float* scale, hipStream_t s);
// RMSNorm(q), RMSNorm(k) per head + rotary embedding, in place on rows [R][ld] fp16: q heads at columns
// q_col + h*D, k heads at k_col + h*D (D = 128); position of row r = pos0 + r % rps; cos/sin fp32 [pos][D].
hipError_t launch_qk_norm_rope(half_t* x, int ld, int R, int heads, int D, int q_col, int k_col, const float* wq,
                               const float* wk, float eps, const float* cos_t, const float* sin_t, int pos0, int rps,
                               hipStream_t s, int bf16 = 0);
// FluxPosEmbed: ids fp32 [S][n_axes] -> cos/sin fp32 [S][sum(axes_dim)] (float64 angles, repeat-interleaved pairs)
hipError_t launch_rope_table(const float* ids, int S, int n_axes, const int* axes_dim, double theta, float* cos_t,
                             float* sin_t, int row0, hipStream_t s);
// in-place row softmax of fp16 scores: x[r][0..n) = softmax(scale * x[r][0..n)) (fp32 math), rows of ld halves
hipError_t launch_softmax_rows(half_t* x, int ld, int R, int n, float scale, hipStream_t s);
// VAE tail: moments = quant_conv(h) (1x1, [2L][2L] fp16 weights, fp32 bias or NULL = 0; wq == NULL: identity), mean / logvar split,
// logvar clamp(-30, 20), z = mean + exp(0.5 logvar) * eps (eps == NULL: mode), lat = scaling * z,
// out = in_scale * (noise_a * lat + noise_b * noise) (noise == NULL: no noise) -> NCHW fp16 (B, L, H, W).  h: fp32 [B*HW][2L].
hipError_t launch_vae_finish(const float* h, int B, int HW, int L, const half_t* wq, const float* bq, const half_t* eps,
                             const half_t* noise, float scaling, float noise_a, float noise_b, float in_scale, half_t* out,
                             hipStream_t s);
// The same tail for K timesteps of the same images (1 <= K <= GDF_MAX_TIMESTEPS): moments and quant_conv once per (image, pixel), then for every k
// row r = k * B + b of eps / noise / out — each NCHW fp16, row block k starting k * t_stride ELEMENTS after block 0 (t_stride >= B * L * HW;
// == for one pass over the whole batch, larger for a sub-batch pass of a bigger batch) — with the k-th (noise_a, noise_b, in_scale).
// The three arrays are HOST pointers of K floats; they travel in the kernel arguments (VaeTimesteps).  Per element the arithmetic is
// launch_vae_finish's, bit for bit.
struct VaeTimesteps { float noise_a[GDF_MAX_TIMESTEPS], noise_b[GDF_MAX_TIMESTEPS], in_scale[GDF_MAX_TIMESTEPS]; };
hipError_t launch_vae_finish_multi(const float* h, int B, int HW, int L, const half_t* wq, const float* bq, const half_t* eps,
                                   const half_t* noise, float scaling, int K, const float* noise_a, const float* noise_b,
                                   const float* in_scale, half_t* out, long t_stride, hipStream_t s);
// The Flux latent-preparation tail (1 <= L <= 16, H and W even): the same moments, out = noise_a * scaling * ((mean - shift) + std * eps) +
// noise_b * noise — vae_finish's value on (mean - shift) with in_scale = 1 — written 2x2-PACKED: (B, (H/2)(W/2), 4L) fp16 or bf16 (out_bf16), element
// [b][gy * (W/2) + gx][c * 4 + dy * 2 + dx] = latent (b, c, 2gy + dy, 2gx + dx) (FluxImg2ImgPipeline._pack_latents).  eps / noise NCHW fp16 or NULL.
// L > 16, odd H or W, a null h / out: hipErrorInvalidValue, nothing launched.
hipError_t launch_vae_finish_packed(const float* h, int B, int H, int W, int L, const half_t* wq, const float* bq, const half_t* eps,
                                    const half_t* noise, float scaling, float shift, float noise_a, float noise_b, int out_bf16, void* out,
                                    hipStream_t s);
// VAE decoder head: z = (c_sample * latents + c_eps * noise_pred) * inv_scaling; y = post_quant_conv(z) (wq == NULL: identity)
// -> NHWC fp16 padded to 8 channels.  latents / noise_pred NCHW fp16 (B, L, H, W); noise_pred may be NULL (plain decode)
hipError_t launch_vae_dec_prepare(const half_t* lat, const half_t* eps, int B, int HW, int L, float ca, float cb, float inv_sf,
                                  const half_t* wq, const float* bq, half_t* nhwc8, hipStream_t s);
// PatchEmbed positional table (embeddings.get_2d_sincos_pos_embed as PatchEmbed calls it): out fp32 [gh*gw][C]
hipError_t launch_sincos_pos_embed(float* out, int C, int gh, int gw, int base_size, float interpolation_scale, hipStream_t s);
// out[b][i] = table[i] + vec[b][i % period]   (ada_norm_single: scale_shift_table + timestep embedding, all blocks at once)
hipError_t launch_add_table(const float* table, const float* vec, int ldvec, int period, int B, long n, float* out, long ldo,
                            hipStream_t s);
// latents NCHW fp16 (B,Cin,H,W) -> patch rows [B*(H/p)*(W/p)][kpad] fp16, column = (c*p + py)*p + px (Conv2d weight order), zero padded
hipError_t launch_patchify(const half_t* x, int B, int Cin, int H, int W, int p, int kpad, half_t* out, hipStream_t s);
// token rows [B*gh*gw][p*p*Cout] fp16 -> NCHW fp16 (B,Cout,gh*p,gw*p)  (transformer_2d.py:563-570 einsum nhwpqc->nchpwq)
hipError_t launch_unpatchify(const half_t* x, int B, int Cout, int gh, int gw, int p, half_t* out, hipStream_t s);
// dst[r][0..kdst) = src[r][0..ksrc) zero padded (weights whose K is not a multiple of 64: the 2x2 patch conv)
hipError_t launch_relayout_rows_padk(const void* src, int src_f32, half_t* dst, int R, int ksrc, int kdst, hipStream_t s);
// out[i] = silu(x[i])
hipError_t launch_silu_vec(const float* x, float* out, long n, hipStream_t s);
// scheduler update between two forwards of a latent trajectory (dit.hip): x' = c_sample x + c_eps eps on the fp32 master, the next forward's fp16
// input c_in x' and timestep; the coefficient row is picked by the device-side step counter at the head of `steps`
hipError_t launch_latent_step(float* x, const half_t* eps, half_t* y, float* tbuf, int* steps, int B, int H, int W, int prime, hipStream_t s);
// the update between two forwards of a guided sampling run (dit.hip): e = e_u + g (e_c - e_u) into a ring of the last five, x' = c_sample x +
// sum_j w_j e_{k-j} on the fp32 master (B samples), the next forward's fp16 input (both halves when guided) and timestep; row, guidance scale
// and the guided flag come from the `steps` block on the device
hipError_t launch_guided_step(float* x, const half_t* eps, float* hist, half_t* y, float* tbuf, int* steps, int B, int H, int W, int prime,
                              hipStream_t s);
// strided 2-D copy with cast to fp16: dst[r][c] = src[r][c]   (hook stores)
// src_bf16: s16 holds bf16; sat: clamp to the fp16 range instead of producing +-inf (hook stores of the bf16 / MMDiT path)
// s_lo > 0: the 16-bit source is a split pair (lo s_lo elements after hi in the row): dst = fp16(hi + lo)
hipError_t launch_copy2d(const half_t* s16, const float* s32, int lds_, half_t* dst, int ldd, int R, int C,
                         hipStream_t s, int src_bf16 = 0, int sat = 0, int s_lo = 0, float scale = 1.0f);   // scale != 1: dst = fp16(scale * src)
// latents NCHW fp16 (B,Cin,H,W) -> NHWC padded to 8 channels (conv_in operand) and optional NHWC hook copy
hipError_t launch_pack_latents(const half_t* x, int B, int Cin, int H, int W, half_t* nhwc8, half_t* hook_nhwc,
                               hipStream_t s);
// sinusoidal embedding: out[b][off + j] (dim entries, [cos|sin] order = flip_sin_to_cos) of t[b*tstride + ti]
// tscale multiplies t first (Flux: `timestep * 1000`, transformer_flux.py:472)
hipError_t launch_sinusoid(const float* t, int B, int n_per_row, int dim, float* out, int ldo, int col_off,
                           int round_f16, hipStream_t s, float tscale = 1.0f);
// widen fp16 vector rows into fp32: out[b][col_off + j] = x[b][j]
hipError_t launch_widen(const half_t* x, int B, int n, float* out, int ldo, int col_off, hipStream_t s, int src_bf16 = 0);
// small-M linear in fp32 vectors: out[m][n] = (accum? out : 0) + bias[n] + sum_k act(x[m][k]) * W[n][k]
hipError_t launch_small_linear(const float* x, int ldx, int M, int K, const half_t* Wt, const float* bias, int N,
                               int silu_in, int accumulate, float* out, int ldo, hipStream_t s, int w_bf16 = 0);

// ------------------------------------------------------------------------------------------------
// output-stage post-processing (csrc/post.hip): `--aggregate_output`, `feature_resize`, aggregated attention feature
// ------------------------------------------------------------------------------------------------
// nearest-resize one layer (logical (B,C,H,W), element strides sb/sc/sy/sx, fp16 or fp32) to S x S and store it as channels
// [coff, coff + C) of out (B, Ctot, S, S) fp16 contiguous
hipError_t launch_resize_concat(const half_t* s16, const float* s32, long sb, long sc, long sy, long sx, int B, int C, int H, int W,
                                half_t* out, int Ctot, int coff, int S, hipStream_t s);
// F.interpolate(v, (OH, OW), mode='bilinear') (align_corners = false, no antialias) of n <= AGG_MAX layers + torch.cat(dim=1) in ONE launch:
// source l is a logical (B, C, H, W) tensor, fp16 or fp32, element strides sb/sc/sy/sx, and lands in channels [coff, coff + C) of
// out (B, Ctot, OH, OW) contiguous, fp16 or fp32.  fp32 coordinates and blend as ATen's upsample_bilinear2d, one rounding to the output type.
enum { AGG_MAX = 16 };
struct AggSrc { const void* ptr; int f32; long sb, sc, sy, sx; int C, H, W, coff; };
hipError_t launch_aggregate(const AggSrc* srcs, int n, int B, void* out, int out_f32, int Ctot, int OH, int OW, hipStream_t s);
// find_nn_source_correspondences (corres.hip): for N source points of f1, the pixel of f2 upsampled (bilinear) to (LH, LW) whose vector has the highest
// cosine similarity, without either upsampled map: out_yx (B, N, 2) int64 (y, x), out_score (B, N) fp32.  f1 / f2 are logical (B, C, H, W) tensors
// (coff unused); points (B, N, 2) fp32 on the device; queries go in chunks of NN_MAXQ; workspace of nn_match_workspace bytes, 16-byte aligned.
enum { NN_MAXQ = 24, NN_FINE_BLOCKS = 1024 };
size_t nn_match_workspace(int B, int N, int C, int h2, int w2);
hipError_t launch_nn_match(const AggSrc& f1, const AggSrc& f2, int B, const float* points, int N, int LH, int LW, long long* out_yx,
                           float* out_score, void* workspace, hipStream_t s);
// batch_cosine_sim + find_nn_correspondences / the two torch.max of find_best_buddies_correspondences (densematch.hip): for every pixel of f1 the pixel
// of f2 with the highest cosine similarity and that cosine (nn12, sim12: (B, P1)), and the reverse (nn21, sim21: (B, P2)), from one MFMA pass over the
// P1 x P2 matrix, which is never written.  f1 / f2 are logical (B, C, H, W) tensors (coff unused), P = H * W; either output pair may be null.  The
// matrix is tiled DM_TILE x DM_TILE, C is padded to DM_KPAD; workspace of dense_match_workspace bytes, 16-byte aligned.
enum { DM_TILE = 256, DM_KPAD = 64, DM_GROUP = 8, DM_MAXP = 1 << 30 };
size_t dense_match_workspace(int B, int C, long P1, long P2, int f32_1, int f32_2);
hipError_t launch_dense_match(const AggSrc& f1, const AggSrc& f2, int B, int* nn12, float* sim12, int* nn21, float* sim21, void* workspace,
                              hipStream_t s);
// compute_clip_loss of the correspondence evaluator (cliploss.hip): the symmetric cross-entropy of scale * cosine similarity between N source pixels of
// f1 and N target pixels of f2 (flat indices (B, N) int64 on the device), without either P x P similarity matrix, and its gradient with respect to
// both maps.  loss (B) fp32, terms (B, 2, N) fp32 or null.  The forward leaves the backward's state (cos, inverse norms, log-sum-exps, validity) in
// the workspace (clip_loss_workspace bytes, 16-byte aligned); the backward takes the same arguments and that workspace, grad_loss (B) on the device,
// and writes grad_f1 / grad_f2 (B, C, H, W) fp32 contiguous (either may be null).  Queries go in chunks of CL_MAXQ; a map's pixels are split into at
// most CL_RANGES ranges whose partial sums the workspace holds.
enum { CL_MAXQ = 24, CL_RANGES = 16 };
size_t clip_loss_workspace(int B, int N, int C, int P1, int P2);
hipError_t launch_clip_loss(const AggSrc& f1, const AggSrc& f2, int B, const long long* src_idx, const long long* tgt_idx, int N, float scale,
                            float* loss, float* terms, void* workspace, hipStream_t s);
hipError_t launch_clip_loss_backward(const AggSrc& f1, const AggSrc& f2, int B, const long long* src_idx, const long long* tgt_idx, int N,
                                     float scale, const float* grad_loss, float* grad_f1, float* grad_f2, void* workspace, hipStream_t s);
// PCA of a feature map (pca.hip): the k <= 8 leading principal components of the (H W, C) samples of every image, or of the (B H W, C) samples of
// the batch (joint): mean (G, C), components (G, k, C), variance (G, k), total_variance (G), projection (B, k, H, W) or null, info (G, 2) int32
// (iterations, converged), all fp32 but info; G = joint ? 1 : B.  Centred covariance on the MFMA units from fp16 (hi, lo) pairs, block subspace
// iteration with 8 vectors and a Rayleigh-Ritz step per iteration, every iteration enqueued.  workspace: pca_workspace bytes, 16-byte aligned.
// launch_pca_rgb: the reference's picture of a (B, 3, H, W) projection -> (B, OH, OW, 3) uint8.
enum { PCA_MAXC = 4096, PCA_MAXITER = 1024 };
size_t pca_workspace(int B, int C, int H, int W, int joint);
hipError_t launch_pca(const AggSrc& f, int B, int k, int joint, int max_iter, float tol, float* mean, float* components, float* variance,
                      float* total_variance, float* projection, int* info, void* workspace, hipStream_t s);
hipError_t launch_pca_rgb(const float* projection, int B, int H, int W, int joint, unsigned char* out, int OH, int OW, hipStream_t s);
// predict_labels of the label-scarce segmentation evaluator (pixcls.hip): an ensemble of M BatchNorm-folded per-pixel MLPs C -> h1 -> h2 -> K over
// every pixel of a logical (B, C, H, W) map, then the per-pixel vote.  pixcls_create packs W1 and W2 as scaled fp16 (hi, lo) pairs in MFMA fragment order
// and uploads everything once (host fp32 arrays: W1 (M, h1, C), b1 (M, h1), W2 (M, h2, h1), b2 (M, h2), W3 (M, K, h2), b3 (M, K)); widths are
// padded with zero weights to (H1P, H2P) = (128, 32) or (256, 128).  launch_pixcls: fp32 logits (M, P, K), P = B * H * W, go to `logits` or, if null,
// to the workspace (pixcls_workspace bytes, 16-byte aligned); labels (P) int64, js (P) fp32 or null, model_labels (M, P) uint8 or null.
enum { PC_MAXM = 16, PC_MAXK = 64, PC_MAXH = 256 };
struct PixCls {
  int C, M, h1, h2, K, H1P, H2P, nkt;
  void* dev;
  const void* w1; const float *inv_s, *b1; const void* w2; const float *inv_s2, *b2, *w3, *b3;
};
hipError_t pixcls_create(int C, int M, int h1, int h2, int K, const float* W1, const float* b1, const float* W2, const float* b2,
                         const float* W3, const float* b3, PixCls** out);
void pixcls_destroy(PixCls* pc);
size_t pixcls_workspace(const PixCls* pc, long P);
hipError_t launch_pixcls(const PixCls* pc, const AggSrc& x, int B, long long* labels, float* js, unsigned char* model_labels, float* logits,
                         void* workspace, hipStream_t s);
// the output convolution of the correspondence evaluator's aggregation network (agghead.hip): 3 x 3, stride 1, zero padding 1, fp32 result, on a
// logical (B, Cin, H, W) map.  agghead_create packs the host fp32 OIHW weights (Cout, Cin, 3, 3) as row-scaled fp16 (hi, lo) pairs in MFMA fragment
// order, one 32-row block at a time, and uploads them with 1 / scale and the bias (null: zeros) per output channel; the packed image is addressed
// with 64-bit offsets (7360 -> 3680 is close to 1 GB).  launch_agghead: out (B, Cout, H, W) fp32 contiguous; B * H * W < 2^31.
// agghead_update repacks fp32 OIHW weights that live on the device into h's image and 1 / scale in place (two launches on `s`, no allocation, no
// host synchronisation; for finite weights the same bits agghead_create packs on the host); agghead_create_device
// is the allocation, the bias (device, or null: zeros) and the same kernels.
struct AggHead {
  int Cin, Cout, nkt, nrb;
  void* dev;
  const void* w; const float *inv_s, *bias;
};
hipError_t agghead_create(int Cin, int Cout, const float* W, const float* bias, AggHead** out);
hipError_t agghead_create_device(int Cin, int Cout, const float* W_dev, const float* bias_dev, hipStream_t s, AggHead** out);
hipError_t agghead_update(AggHead* h, const float* W_dev, hipStream_t s);
void agghead_destroy(AggHead* h);
hipError_t launch_agghead(const AggHead* h, const AggSrc& x, int B, float* out, hipStream_t s);
// the weight gradient of that convolution (aggwgrad.hip): dW (Cout, x.C, 3, 3) fp32 OIHW = sum over (b, y, x) of grad_out (B, Cout, H, W) fp32
// contiguous times the shifted map x (logical (B, C, H, W), fp16 or fp32, any strides); accumulate: the complete sum is added once to what dW
// holds.  The workspace (agghead_wgrad_workspace bytes, 16-byte aligned) receives max |grad_out| (Cout floats), the shift (Cout ints) per
// output channel and grad_out as scaled fp16 (hi, lo) pairs in MFMA fragment order.  B * H * W < 2^31.
size_t agghead_wgrad_workspace(int B, int Cout, int H, int W);
hipError_t launch_agghead_wgrad(const AggSrc& x, int B, const float* grad_out, int Cout, float* dW, int accumulate, void* workspace, hipStream_t s);
// adaptive_avg_pool2d to (H/r, W/r) of a channels-last hook (B,C,H,W; strides sb, 1, sy, sx) -> (B, H/r, W/r, C) fp16: the r x r mean
// where r divides H and W, ATen's longer windows [floor(o H / OH), ceil((o + 1) H / OH)) otherwise
hipError_t launch_avg_pool(const half_t* src, long sb, long sy, long sx, int B, int C, int H, int W, int r, half_t* out, hipStream_t s);
// mean over heads and over n <= 32 maps (B, heads, Q, K) fp16 -> (B, Q, K) fp32
hipError_t launch_maps_mean(const half_t* const* maps, int n, int B, int heads, int Q, int K, float* out, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// ControlNet conditioning (csrc/control.hip)
// ------------------------------------------------------------------------------------------------
// dst[r][0..C) += res[r][0..C) for up to RES_ADD_MAX tensors in ONE launch: dst fp16 rows of ld elements (a slice of a wider row: the pointer
// carries the column offset), res fp16 contiguous [rows][C]; lo > 0: dst is a split (hi, lo) pair, lo `lo` elements after hi in the same row,
// rewritten as the pair of hi + lo + res (fp32).  C, ld, lo multiples of 8, both pointers 16-byte aligned.
enum { RES_ADD_MAX = 16 };
struct ResAddDesc { half_t* dst; int ld; int lo; const half_t* res; int rows; int C; };
hipError_t launch_residual_add(const ResAddDesc* d, int n, hipStream_t s);

// The conditioning embedding's 3x3 convs, padding 1 (csrc/cond_embed.hip): x NHWC fp16 [B][H][W][ldx >= Cin], w as launch_cond_pack_weights packs
// it, out NHWC fp16 [B][OH][OW][ldo >= Cout], OH = (H - 1) / stride + 1; v = acc + bias, silu: v * sigmoid(v), add: v += out's old value; one
// fp16 rounding.  (Cin, Cout) one of cond_conv_ok()'s pairs, stride 1 | 2 (even H and W at 2), ldx / ldo multiples of 8, pointers 16-byte aligned.
// OH, OW, M and Kpad are filled in by the launcher.
struct CondConvParams {
  const half_t* x; const half_t* w; const float* bias; half_t* out;
  int B, H, W, OH, OW, Cin, ldx, Cout, ldo, stride, silu, add, Kpad; unsigned M;
};
bool cond_conv_ok(int Cin, int Cout);
size_t cond_conv_weight_bytes(int Cin, int Cout);
hipError_t launch_cond_conv3x3(const CondConvParams& p, hipStream_t s);
// OIHW src[O][I][3][3] (dtype 0 fp16, 1 fp32, 2 bf16) -> fp16 [k / 8][O][8], k = tap * cin_pad + c, zero padded to a multiple of 32 in k
hipError_t launch_cond_pack_weights(const void* src, int dtype, half_t* dst, int O, int I, int cin_pad, hipStream_t s);
// control image NCHW (B, C <= 8, H, W) fp16 (dtype 0) or fp32 (1) -> NHWC pixels of 8 fp16 channels, channels from C up zero
hipError_t launch_cond_pack_image(const void* x, int dtype, int B, int C, int H, int W, half_t* nhwc8, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Canny edge detector, the 'canny' / 'canny-xl' ControlNet preprocessor (csrc/canny.hip)
// ------------------------------------------------------------------------------------------------
// src_kind 0 uint8 [B][H][W][3], 1 uint8 [B][H][W], 2 fp32 / 3 fp16 [B][3][H][W] in [-1, 1] (quantised on load); low <= high;
// cls uint8 [B][H][W]: 2 strong, 0 candidate, 1 neither.  B H W < 2^31; src and cls 4-byte aligned.
enum { CANNY_LINK_TILE = 32 };
hipError_t launch_canny_classify(const void* src, int src_kind, int B, int H, int W, int low, int high, uint8_t* cls, hipStream_t s);
// hysteresis: dst_kind 0 uint8 [B][H][W] 0 / 255, 1 fp16 [B][3][H][W] 0.0 / 1.0; four launches; workspace canny_workspace_bytes(), 16-byte aligned
hipError_t launch_canny_link(const uint8_t* cls, int B, int H, int W, void* dst, int dst_kind, void* workspace, hipStream_t s);
size_t canny_workspace_bytes(int B, int H, int W);
uint8_t* canny_workspace_cls(void* workspace, int B, int H, int W);     // the class map of the fused entry, behind the linking stage's part

// ------------------------------------------------------------------------------------------------
// PIL-to-tensor preprocessing: Pillow's 8-bit bicubic resize, convert("RGB"), normalisation (csrc/preproc.hip)
// ------------------------------------------------------------------------------------------------
// One axis' table for `in` source and `out` target samples: bounds int32 [out][2] = (xmin, xmax), kk int32 [out][pil_ksize(in, out)]
int pil_ksize(int in, int out);
hipError_t launch_pil_coeffs(int in, int out, int* bounds, int* kk, hipStream_t s);
// src uint8 [src_h][src_w][C], C 1 or 3, any alignment -> dst_u8 uint8 [out_h][out_w][3] and / or dst_f32 fp32 [3][out_h][out_w] (either may be
// null); workspace pil_resize_workspace_bytes(), 16-byte aligned.  src_h out_w C, 3 out_h out_w < 2^31; in <= 32 out per axis.
hipError_t launch_pil_resize_u8(const uint8_t* src, int src_h, int src_w, int C, int out_h, int out_w, uint8_t* dst_u8, float* dst_f32,
                                void* workspace, hipStream_t s);
size_t pil_resize_workspace_bytes(int src_h, int src_w, int channels, int out_h, int out_w);

// ------------------------------------------------------------------------------------------------
// weight re-layout (model load time)
// ------------------------------------------------------------------------------------------------
// `src_f32` is the source dtype code of gdf_model_set_param: 0 fp16, 1 fp32, 2 bf16
// generic: dst[o][t][i] = src[o][i][t]  (OIHW -> OHWI with T = kh*kw); i padded to ipad, t to tpad
// cblk > 0: dst[o][i / cblk][t][i % cblk] (the 3x3-conv K order of gemm_kernel<A_CONV3>: K index = ((c / 64) * 9 + tap) * 64 + c % 64)
hipError_t launch_relayout_conv(const void* src, int src_f32, half_t* dst, int O, int I, int T, int ipad, int tpad,
                                hipStream_t s, int cblk = 0);
// rows: dst[rowmap(r)][k] = src[r][k] for r in [0,R); rowmap: 0 identity+row_off, 1 GEGLU interleave (half = R/2)
hipError_t launch_relayout_rows(const void* src, int src_f32, half_t* dst, int R, int K, int row_off, int geglu /*0 or interleave group (16)*/,
                                hipStream_t s, int dst_bf16 = 0);
// vectors to fp32 with the same row mapping
hipError_t launch_relayout_vec(const void* src, int src_f32, float* dst, int R, int row_off, int geglu, hipStream_t s);

}  // namespace gdf
